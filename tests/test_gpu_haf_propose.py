"""HAF proposals (mh_propose_haf, mh_get_haf_support; csrc/haf_propose.hip) on the GPU: the single-correspondence batch against
mh_local_homographies bit for bit, the refitted batches and their support masks against the numpy twin
(tests/haf_propose_numpy.py) bit for bit, the resident batch under the scoring and selecting entry points, states and error
codes, the sharded selection, and the host class."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import haf_propose_numpy as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

THR2 = 6.25
INVALID, NOT_SET = -2, -4
_cache = {}


def _scene(mh, n):
    """600: three planes and outliers; the small ones: one plane (5, 33, 63, 64, 65 correspondences)."""
    if ("scene", n) not in _cache:
        _cache["scene", n] = mh.synth.make_scene(n, 3, seed=99, with_neighbours=False) if n == 600 else \
            mh.synth.make_scene(n, 1, seed=5, with_neighbours=False)
    return _cache["scene", n]


def _table(mh, n, k):
    if ("table", n, k) not in _cache:
        sc = _scene(mh, n)
        _cache["table", n, k] = twin.knn_table(sc.src, sc.dst, k)
    return _cache["table", n, k]


def _twin(mh, n, k, members, thr2):
    """The twin's whole batch (stride 1) of scene n over the k-column table: computed once, shared, never changed."""
    key = ("twin", n, k, members, thr2)
    if key not in _cache:
        sc = _scene(mh, n)
        H, used = twin.propose(sc.src, sc.dst, sc.aff, sc.F, sc.e2, 0, sc.n, 1, members, thr2, _table(mh, n, k) if members else None)
        H.setflags(write=False)
        used.setflags(write=False)
        _cache[key] = (H, used)
    return _cache[key]


def _load(engine, sc, k=0):
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_epipolar(sc.F, sc.e2)
    if k:
        engine.build_sample_neighbours(k)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _code(mh, fn):
    with pytest.raises(mh.MultiHError) as ei:
        fn()
    return ei.value.code


# ---- 1. members = 0: the rows of mh_local_homographies --------------------------------------------------------------------
@pytest.mark.parametrize("n", [600, 5, 33, 63, 64, 65])
def test_single_correspondence_batch_is_local_homographies(mh, engine, n):
    sc = _scene(mh, n)
    _load(engine, sc)
    want, _ = engine.local_homographies(0.005)
    engine.propose_haf(0, sc.n, 1, 0, THR2)
    assert engine.model_count == sc.n
    assert np.array_equal(_bits(engine.get_models()), _bits(want))
    assert not engine.get_haf_support().any()
    if n != 600:
        return
    m7 = (sc.n + 6) // 7
    assert m7 == 86
    engine.propose_haf(0, m7, 7, 0, THR2)
    whole7 = engine.get_models()
    assert np.array_equal(_bits(whole7), _bits(want[::7]))
    engine.propose_haf(40, 46, 7, 0, THR2)                       # a shard: counters 40 .. 85 of that batch
    assert engine.model_count == 46
    assert np.array_equal(_bits(engine.get_models()), _bits(whole7[40:]))


@pytest.mark.parametrize("n,k", [(600, 16), (65, 16), (33, 32)])
def test_zero_threshold_is_the_single_correspondence_batch(mh, engine, n, k):
    sc = _scene(mh, n)
    _load(engine, sc, k)
    engine.propose_haf(0, sc.n, 1, 0, 0.0)
    want = engine.get_models()
    engine.propose_haf(0, sc.n, 1, 16, 0.0)
    assert np.array_equal(_bits(engine.get_models()), _bits(want))
    assert not engine.get_haf_support().any()


# ---- 2. refitted batches against the twin ----------------------------------------------------------------------------------
CASES = [(600, 16, 3), (600, 16, 16), (600, 32, 32), (5, 3, 3), (33, 32, 32), (33, 16, 3), (63, 16, 16), (64, 32, 32), (64, 3, 3),
         (65, 16, 16), (65, 32, 32)]      # (n, table k, members): members = 3 also as a prefix of the k = 16 table


@pytest.mark.parametrize("n,k,members", CASES)
@pytest.mark.parametrize("thr2", [THR2, np.inf])
def test_refitted_batch_equals_the_twin(mh, engine, n, k, members, thr2):
    sc = _scene(mh, n)
    _load(engine, sc, k)
    assert np.array_equal(engine.get_sample_neighbours(), _table(mh, n, k))
    want, want_used = _twin(mh, n, k, members, thr2)
    engine.propose_haf(0, sc.n, 1, members, thr2)
    H, used = engine.get_models(), engine.get_haf_support()
    assert np.array_equal(used, want_used)
    finite = np.isfinite(want).all(axis=1)
    print(f"n = {n}, k = {k}, members = {members}, thr2 = {thr2}: twin leaves out {int((~finite).sum())} rows; "
          f"{int((used != 0).sum())} hypotheses refitted, {int(np.unpackbits(used.view(np.uint8)).sum())} consistent neighbours")
    assert (~finite).sum() <= 0.01 * sc.n
    assert np.array_equal(_bits(H[finite]), _bits(want[finite]))
    if n == 600 and members == 16:
        # a strided batch and a shard of it are rows of the whole batch
        engine.propose_haf(0, 86, 7, members, thr2)
        H7, used7 = engine.get_models(), engine.get_haf_support()
        assert np.array_equal(_bits(H7), _bits(H[::7])) and np.array_equal(used7, used[::7])
        engine.propose_haf(40, 46, 7, members, thr2)
        assert np.array_equal(_bits(engine.get_models()), _bits(H7[40:])) and np.array_equal(engine.get_haf_support(), used7[40:])


# ---- 3. the resident batch under the scoring and selecting entry points ------------------------------------------------------
def test_scores_of_the_resident_batch(mh, engine, oracle):
    sc = _scene(mh, 600)
    _load(engine, sc, 16)
    want, _ = _twin(mh, 600, 16, 16, THR2)
    engine.propose_haf(0, sc.n, 1, 16, THR2)
    assert np.array_equal(engine.score(THR2), oracle.score(sc.src, sc.dst, want, THR2))
    cnt, wgt = engine.score_msac(THR2)
    assert np.array_equal(cnt, oracle.score(sc.src, sc.dst, want, THR2)) and (wgt <= 256 * cnt).all()
    best = engine.select_best()
    assert best == (int(np.argmax(cnt)), int(cnt.max()))


@pytest.mark.parametrize("by_weight", [False, True])
def test_selection_over_a_proposed_batch_equals_an_uploaded_one(mh, engine, by_weight):
    sc = _scene(mh, 600)
    _load(engine, sc, 16)
    engine.set_tuning(30, 1)                                      # winners refitted to their inliers
    select = engine.select_greedy_msac if by_weight else engine.select_greedy
    engine.propose_haf(0, sc.n, 1, 16, THR2)
    batch = engine.get_models()
    got = select(THR2, 20, 8, np.ones(sc.n, np.uint8))
    engine.set_models(batch)
    want = select(THR2, 20, 8, np.ones(sc.n, np.uint8))
    assert len(got[1]) >= 3
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    for a, b in zip(got[1:], want[1:]):
        assert np.array_equal(a, b)


# ---- 4. state and errors -----------------------------------------------------------------------------------------------------
def test_arguments(mh, engine):
    sc = _scene(mh, 600)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    assert _code(mh, lambda: engine.propose_haf(0, 10, 1, 0, THR2)) == NOT_SET           # no epipolar geometry
    engine.set_epipolar(sc.F, sc.e2)
    engine.propose_haf(0, 10, 1, 0, THR2)
    assert _code(mh, lambda: engine.propose_haf(0, 10, 1, 16, THR2)) == NOT_SET          # members > 0 without a table
    engine.build_sample_neighbours(16)
    engine.propose_haf(0, 10, 1, 16, THR2)
    engine.propose_haf(0, 10, 1, 3, THR2)
    for first, m, stride, members, thr2 in ((0, 10, 0, 0, THR2), (0, 10, -1, 0, THR2), (0, -1, 1, 0, THR2), (-1, 10, 1, 0, THR2),
                                            (0, 601, 1, 0, THR2), (591, 10, 1, 0, THR2), (0, 87, 7, 0, THR2), (86, 1, 7, 0, THR2),
                                            (1 << 62, 1, 1 << 30, 0, THR2), (0, 10, 1, 1, THR2), (0, 10, 1, 2, THR2),
                                            (0, 10, 1, 17, THR2), (0, 10, 1, 33, THR2), (0, 10, 1, -3, THR2), (0, 10, 1, 0, np.nan)):
        assert _code(mh, lambda: engine.propose_haf(first, m, stride, members, thr2)) == INVALID, (first, m, stride, members, thr2)
    engine.propose_haf(590, 10, 1, 16, THR2)                      # the last ten anchors
    engine.propose_haf(85, 1, 7, 16, THR2)                        # anchor 595
    assert engine.model_count == 1
    # an empty batch: an empty model set, as mh_set_models(NULL, 0) leaves one
    engine.propose_haf(5, 0, 1, 16, THR2)
    assert engine.model_count == 0 and engine.get_haf_support().size == 0
    assert _code(mh, engine.get_models) == NOT_SET
    # affinities missing
    engine.set_correspondences(sc.src, sc.dst)
    assert _code(mh, lambda: engine.propose_haf(0, 10, 1, 0, THR2)) == NOT_SET


def test_what_replaces_the_batch_and_what_goes_stale(mh, engine):
    sc = _scene(mh, 600)
    _load(engine, sc, 16)
    engine.propose_dlt4(1, 0, 50)
    assert _code(mh, engine.get_haf_support) == NOT_SET
    engine.get_samples()
    engine.score_msac(THR2)
    engine.select_best_msac()
    engine.propose_haf(0, 50, 1, 16, THR2)
    assert _code(mh, engine.select_best_msac) == NOT_SET          # the weights belonged to the DLT batch
    assert _code(mh, engine.get_samples) == NOT_SET               # as after mh_set_models
    assert engine.get_haf_support().shape == (50,)
    H = engine.get_models()
    engine.set_models(H)
    assert _code(mh, engine.get_haf_support) == NOT_SET
    engine.propose_haf(0, 50, 1, 16, THR2)
    engine.get_haf_support()
    engine.propose_dlt4(1, 0, 50)
    assert _code(mh, engine.get_haf_support) == NOT_SET
    engine.propose_haf(0, 50, 1, 16, THR2)
    engine.prefetch_dlt4(1, 0, 50)
    engine.adopt_prefetched()
    assert _code(mh, engine.get_haf_support) == NOT_SET
    # new correspondences drop the table: members > 0 answers NOT_SET again, members = 0 still works
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    assert _code(mh, lambda: engine.propose_haf(0, 50, 1, 16, THR2)) == NOT_SET
    engine.propose_haf(0, 50, 1, 0, THR2)


def test_the_residual_mode_does_not_reach_the_consistency_test(mh, engine):
    sc = _scene(mh, 600)
    _load(engine, sc, 16)
    engine.set_residual_mode(True)
    engine.propose_haf(0, sc.n, 1, 16, THR2)
    want, want_used = _twin(mh, 600, 16, 16, THR2)
    assert np.array_equal(engine.get_haf_support(), want_used)
    assert np.array_equal(_bits(engine.get_models()), _bits(want))


# ---- 5. sharded --------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_selection_over_a_haf_batch(mh, engine):
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "haf_propose_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)          # a stranded rank would run into these
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda d: d["rank"])
    assert [d["rank"] for d in recs] == [0, 1]
    # the single-rank calls over the same 600 hypotheses
    sc = _scene(mh, 600)
    engine.set_params(2.6, 2.5, 0.005, 0.5, 20)
    _load(engine, sc, 16)
    for name, refit in (("haf", 0), ("haf_refit", 1), ("haf_again", 0)):
        engine.set_tuning(30, refit)
        engine.propose_haf(0, sc.n, 1, 16, THR2)
        H, counters, counts, _ = engine.select_greedy(THR2, 20, 8, np.ones(sc.n, np.uint8))
        assert len(counters) >= 3
        for rr in recs:
            assert rr[name]["ok"], rr[name]
            assert rr[name]["counters"] == counters.tolist() and rr[name]["counts"] == counts.tolist(), name
            assert rr[name]["H"] == H.view(np.uint64).tolist(), name
    for name in ("mixed", "other_members"):
        for rr in recs:
            assert not rr[name]["ok"] and rr[name]["code"] == INVALID and "same residual mode" in rr[name]["msg"], rr[name]
            assert "mh_propose_haf" in rr[name]["msg"]
    # the host class with one hypothesis for two ranks (rank 1's shard is empty): the unsharded result on both ranks
    for rr in recs:
        assert rr["class_unsharded"]["k"] >= 1, rr["class_unsharded"]["k"]
        assert rr["class_empty_shard"] == rr["class_unsharded"] == recs[0]["class_unsharded"]


# ---- 6. the host class -------------------------------------------------------------------------------------------------------
def _run_process(mh, host, sc, seed=5, hypotheses=4000, max_models=16):
    dp = C.POINTER(C.c_double)
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((64, 9))
    it, en = C.c_int(-1), C.c_double(-1)
    src, dst, aff, F, e2 = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff, sc.F, sc.e2))
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, F.ctypes.data_as(dp),
                             e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.5), C.c_double(0.005), C.c_double(0.5), 20,
                             C.c_ulonglong(seed), hypotheses, max_models, 0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 64, C.byref(it), C.byref(en), None, 0, 4)
    C.CDLL(None).fflush(None)
    return k, labels, Hout[:max(k, 0)].copy()


def test_process_with_haf_proposals(mh, engine_lib, capfd, monkeypatch):
    monkeypatch.setenv("MULTIH_TIMING", "1")                      # the stage log, which names the initial batch
    sc = mh.synth.make_scene(2000, 5, seed=99)
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    default = _run_process(mh, host, sc)
    assert "HAF proposals" not in capfd.readouterr().out
    planes_default = mh.synth.agreement(sc.gt_label, default[1])["planes_recovered"]
    try:
        for members, stride in ((16, 1), (16, 4)):
            host.mhh_set_proposal_source(1, members, stride)
            k, labels, H = _run_process(mh, host, sc)
            log = capfd.readouterr().out
            hypotheses = (sc.n + stride - 1) // stride
            assert f"[Multi-H] HAF proposals: {hypotheses} hypotheses (members {members}, stride {stride}); SetProposal's count of 4000 is ignored" in log
            assert "initial models done" in log
            assert k >= 2 and labels.min() >= -1 and labels.max() < k
            got = mh.synth.agreement(sc.gt_label, labels)
            print(f"HAF ({members}, {stride}): {hypotheses} hypotheses, {k} models, planes {got['planes_recovered']} of {got['planes']} "
                  f"(default route {planes_default}), ARI {got['ari']:.4f}")
            assert got["planes_recovered"] >= planes_default
    finally:
        host.mhh_set_proposal_source(0, 16, 1)
    # the source is not sticky on a pooled engine: the default route is what it was
    again = _run_process(mh, host, sc)
    assert "HAF proposals" not in capfd.readouterr().out
    assert again[0] == default[0] and np.array_equal(again[1], default[1])
    assert np.array_equal(again[2].view(np.uint64), default[2].view(np.uint64))
