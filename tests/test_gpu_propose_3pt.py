"""3-point proposals (mh_propose_3pt; csrc/propose3pt.hip) on the GPU: batches and tuples against the twin
(tests/propose_3pt_numpy.py: the samplers' tuples, the host library's Homography3PTLinear on the CPU) bit for bit, degenerate
tuples, the local sampler, states and error codes, the resident batch under the scoring and selecting entry points, the sharded
selection, and the host class."""
import ctypes as C
import itertools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import msac_numpy as W
import propose_3pt_numpy as twin
import select_msac_numpy as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

THR2 = 2.5 ** 2
NEED, MAX_MODELS = 20, 8
UNIFORM, LOCAL = 0, 1
INVALID, NOT_SET = -2, -4
SEED = 77
WRAP_FIRST, WRAP_SEED = (1 << 56) - 2, 1000        # (c << 8) passes 2^64 inside the batch, and seed + (c << 8) just before it
QNAN = 0x7ff8000000000000
_cache = {}


def _scene(mh, n=600):
    if n not in _cache:
        _cache[n] = mh.synth.make_scene(n, 3, seed=99, with_neighbours=False)
    return _cache[n]


def _batch(mh, seed, first, m, nbr_k=0, u=0):
    """The twin's batch of the 600-point scene: (H, samples); computed once per key, shared, never changed."""
    key = ("batch", seed, first, m, nbr_k, u)
    if key not in _cache:
        sc = _scene(mh)
        nbr = _table(mh, nbr_k) if nbr_k else None
        H, smp = twin.propose(twin.host_lib(mh.LIB_PATH), sc.src, sc.dst, sc.F, seed, first, m, nbr, u)
        H.setflags(write=False)
        smp.setflags(write=False)
        _cache[key] = (H, smp)
    return _cache[key]


def _table(mh, k):
    if ("table", k) not in _cache:
        sc = _scene(mh)
        _cache["table", k] = twin.knn_table(sc.src, sc.dst, k)
    return _cache["table", k]


def _load(engine, sc):
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_epipolar(sc.F, sc.e2)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _code(mh, fn):
    with pytest.raises(mh.MultiHError) as ei:
        fn()
    return ei.value.code


# ---- 1. the batch, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,first", [(SEED, 0), (WRAP_SEED, WRAP_FIRST)])
def test_batch_equals_the_twin(mh, engine, seed, first):
    sc = _scene(mh)
    _load(engine, sc)
    want, want_idx = _batch(mh, seed, first, 1000)
    assert np.isfinite(want).all(axis=1).sum() >= 990
    for m in (1000, 1, 63, 64, 65, 130):                       # one lane per hypothesis, 64-lane workgroups
        engine.propose_3pt(seed, first, m)
        assert engine.model_count == m
        idx = engine.get_samples()
        assert idx.shape == (m, 4) and np.array_equal(idx, want_idx[:m]) and (idx[:, 3] == -1).all(), (seed, first, m)
        assert np.array_equal(_bits(engine.get_models()), _bits(want[:m])), (seed, first, m)
    # a shard of the batch is rows of the batch: counters are global
    engine.propose_3pt(seed, first + 700, 300)
    assert np.array_equal(engine.get_samples(), want_idx[700:]) and np.array_equal(_bits(engine.get_models()), _bits(want[700:]))


# ---- 2. degenerate tuples -----------------------------------------------------------------------------------------------------
def _degenerate_set(mh):
    """Eight rows: three collinear source points, two identical correspondences, a destination point on the epipole, a row of
    zeros — the four cases the issue names: every triple of them fits FINITE, on the host and on the device alike (rank-deficient
    normal equations lose an eigenvalue, they do not overflow) — and, added here so that failed fits exist at all, a row whose
    squares overflow (1e200): no 3-point fit survives it, and all failures come from the 21 of the 56 triples that hold it."""
    sc = _scene(mh)
    src, dst = sc.src[:8].copy(), sc.dst[:8].copy()
    src[0], src[1], src[2] = (100.0, 100.0), (200.0, 200.0), (300.0, 300.0)
    src[4], dst[4] = src[3], dst[3]
    dst[5] = sc.e2
    src[6], dst[6] = 0.0, 0.0
    src[7], dst[7] = (1e200, -1e200), (1e200, 1e200)
    return src, dst, sc.F, sc.e2


def test_degenerate_tuples(mh, engine):
    src, dst, F, e2 = _degenerate_set(mh)
    host = twin.host_lib(mh.LIB_PATH)
    idx3 = twin.tuples(3, 0, 2000, 8)
    assert {tuple(sorted(t)) for t in idx3.tolist()} == set(itertools.combinations(range(8), 3)), "every one of the 56 triples"
    with np.errstate(all="ignore"):
        want, ok = twin.fit(host, src, dst, F, idx3)
    engine.set_correspondences(src, dst)
    engine.set_epipolar(F, e2)
    engine.propose_3pt(3, 0, 2000)
    H = engine.get_models()
    assert np.array_equal(engine.get_samples(), twin.samples(idx3))
    failed = np.isnan(H).all(axis=1)
    print(f"{int(failed.sum())} of 2000 fits failed on the device, {int((~ok).sum())} on the host")
    assert np.array_equal(failed, ~ok) and failed.any() and not failed.all()
    assert (_bits(H[failed]) == QNAN).all()
    assert np.isfinite(want[ok]).all() and np.array_equal(_bits(H[ok]), _bits(want[ok]))
    assert (engine.score(THR2)[failed] == 0).all()
    # three correspondences: one possible set of indices
    engine.set_correspondences(src[:3], dst[:3])
    engine.set_epipolar(F, e2)
    engine.propose_3pt(5, 0, 100)
    idx = engine.get_samples()
    assert np.array_equal(idx, twin.samples(twin.tuples(5, 0, 100, 3))) and (np.sort(idx[:, :3], axis=1) == [0, 1, 2]).all()
    want3, _ = twin.fit(host, src[:3], dst[:3], F, idx[:, :3])
    assert np.array_equal(_bits(engine.get_models()), _bits(want3))
    engine.set_correspondences(src[:2], dst[:2])
    engine.set_epipolar(F, e2)
    assert _code(mh, lambda: engine.propose_3pt(5, 0, 100)) == INVALID


# ---- 3. the local sampler -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,first", [(SEED, 0), (WRAP_SEED, WRAP_FIRST)])
def test_local_sampler(mh, engine, seed, first):
    sc = _scene(mh)
    _load(engine, sc)
    engine.build_sample_neighbours(8)
    assert np.array_equal(engine.get_sample_neighbours(), _table(mh, 8))
    for u in (0, 4, 16):
        want, want_idx = _batch(mh, seed, first, 1000, 8, u)
        engine.set_sampler(LOCAL, u)
        for m in (1000, 65):
            engine.propose_3pt(seed, first, m)
            assert np.array_equal(engine.get_samples(), want_idx[:m]), (u, m)
            assert np.array_equal(_bits(engine.get_models()), _bits(want[:m])), (u, m)
    uni, uni_idx = _batch(mh, seed, first, 1000)
    assert np.array_equal(want_idx, uni_idx) and np.array_equal(_bits(want), _bits(uni)), "all 16 of 16 uniform: the uniform batch"
    assert not np.array_equal(_batch(mh, seed, first, 1000, 8, 0)[1], uni_idx)
    engine.set_sampler(UNIFORM, 0)
    engine.propose_3pt(seed, first, 1000)
    assert np.array_equal(engine.get_samples(), uni_idx)


# ---- 4. state and errors ------------------------------------------------------------------------------------------------------
def test_state_and_errors(mh, engine):
    sc = _scene(mh)
    assert _code(mh, lambda: engine.propose_3pt(1, 0, 10)) == NOT_SET            # no correspondences
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    assert _code(mh, lambda: engine.propose_3pt(1, 0, 10)) == NOT_SET            # no epipolar geometry
    engine.set_epipolar(sc.F, sc.e2)
    engine.propose_3pt(1, 0, 10)
    for first, m in ((0, -1), (-1, 10)):
        assert _code(mh, lambda: engine.propose_3pt(1, first, m)) == INVALID, (first, m)
    engine.set_sampler(LOCAL, 4)
    assert _code(mh, lambda: engine.propose_3pt(1, 0, 10)) == NOT_SET            # the local sampler without its table
    engine.set_sampler(UNIFORM, 0)
    # an empty batch: an empty model set, as mh_set_models(NULL, 0) leaves one
    engine.propose_3pt(1, 5, 0)
    assert engine.model_count == 0
    assert _code(mh, engine.get_models) == NOT_SET
    # what goes stale: the MSAC weights and the HAF record of the batch before
    engine.build_sample_neighbours(16)
    engine.propose_haf(0, 50, 1, 16, THR2)
    engine.get_haf_support()
    engine.score_msac(THR2)
    engine.select_best_msac()
    engine.propose_3pt(1, 0, 50)
    assert _code(mh, engine.select_best_msac) == NOT_SET
    assert _code(mh, engine.get_haf_support) == NOT_SET
    assert np.array_equal(engine.get_samples(), _batch(mh, 1, 0, 50)[1])
    # the next DLT batch has its own tuples again
    engine.propose_dlt4(1, 0, 50)
    import oracle_lib
    dlt_idx = engine.get_samples()
    assert np.array_equal(dlt_idx, oracle_lib.sample4(1, 0, 50, sc.n)) and (dlt_idx[:, 3] >= 0).all()
    assert np.array_equal(dlt_idx[:, :3], _batch(mh, 1, 0, 50)[1][:, :3])
    # an uploaded set has none
    engine.propose_3pt(1, 0, 50)
    engine.set_models(engine.get_models())
    assert _code(mh, engine.get_samples) == NOT_SET


# ---- 5. the resident batch under the scoring and selecting entry points -------------------------------------------------------
@pytest.mark.parametrize("key15", [1, 0])
def test_scores_of_the_resident_batch(mh, engine, oracle, key15):
    sc = _scene(mh)
    _load(engine, sc)
    want, _ = _batch(mh, SEED, 0, 1000)
    engine.set_tuning(15, key15)
    engine.propose_3pt(SEED, 0, 1000)
    counts = oracle.score(sc.src, sc.dst, want, THR2)
    assert np.array_equal(engine.score(THR2), counts)
    cnt, wgt = engine.score_msac(THR2)
    cnt_t, wgt_t = W.score_msac(sc.src, sc.dst, want, THR2)
    assert np.array_equal(cnt, cnt_t) and np.array_equal(wgt, wgt_t) and np.array_equal(cnt, counts)
    assert engine.select_best() == (int(np.argmax(counts)), int(counts.max()))


@pytest.mark.parametrize("key36", [1, 0])
@pytest.mark.parametrize("refit", [0, 1])
def test_selections_over_the_resident_batch(mh, engine, oracle, refit, key36):
    sc = _scene(mh)
    _load(engine, sc)
    want, _ = _batch(mh, SEED, 0, 1000)
    ones = np.ones(sc.n, np.uint8)
    engine.set_tuning(30, refit)
    engine.set_tuning(36, key36)
    fit = T.haf_refit(sc.src, sc.dst, sc.aff, sc.F, sc.e2) if refit else None
    # by count
    engine.propose_3pt(SEED, 0, 1000)
    H, counters, counts, mask = engine.select_greedy(THR2, NEED, MAX_MODELS, ones)
    assert len(counters) >= 3
    if refit:
        H_t, idx_t, cnt_t, _, mask_t = T.select_greedy(sc.src, sc.dst, want, THR2, NEED, MAX_MODELS, rank_by="count", refit=fit)
    else:
        H_t, idx_t, cnt_t, mask_t = oracle.select_greedy(sc.src, sc.dst, want, THR2, NEED, MAX_MODELS)
        assert np.array_equal(_bits(H), _bits(H_t))
    assert np.array_equal(counters, idx_t) and np.array_equal(counts, cnt_t) and np.array_equal(mask, mask_t)
    # by weight
    engine.propose_3pt(SEED, 0, 1000)
    Hw, counters_w, counts_w, weights_w, mask_w = engine.select_greedy_msac(THR2, NEED, MAX_MODELS, ones)
    H_t, idx_t, cnt_t, wgt_t, mask_t = T.select_greedy(sc.src, sc.dst, want, THR2, NEED, MAX_MODELS, rank_by="weight", refit=fit)
    assert np.array_equal(counters_w, idx_t) and np.array_equal(counts_w, cnt_t) and np.array_equal(weights_w, wgt_t)
    assert np.array_equal(mask_w, mask_t)
    if not refit:
        assert np.array_equal(_bits(Hw), _bits(H_t))
    # ... and either way what the same entry points make of the twin's batch uploaded: the proposer leaves nothing else behind
    engine.set_models(want)
    up = engine.select_greedy(THR2, NEED, MAX_MODELS, ones)
    assert np.array_equal(_bits(up[0]), _bits(H)) and all(np.array_equal(a, b) for a, b in zip(up[1:], (counters, counts, mask)))
    engine.set_models(want)
    up = engine.select_greedy_msac(THR2, NEED, MAX_MODELS, ones)
    assert np.array_equal(_bits(up[0]), _bits(Hw))
    assert all(np.array_equal(a, b) for a, b in zip(up[1:], (counters_w, counts_w, weights_w, mask_w)))


def test_refitted_winners_under_the_3pt_estimator(mh, engine):
    sc = _scene(mh)
    engine.set_correspondences(sc.src, sc.dst)                   # point-only: no affinities anywhere
    engine.set_epipolar(sc.F, sc.e2)
    engine.set_estimator("3pt")
    engine.set_tuning(30, 1)
    ones = np.ones(sc.n, np.uint8)
    engine.propose_3pt(SEED, 0, 1000)
    got = engine.select_greedy(THR2, NEED, MAX_MODELS, ones)
    engine.set_models(_batch(mh, SEED, 0, 1000)[0])
    want = engine.select_greedy(THR2, NEED, MAX_MODELS, ones)
    assert len(got[1]) >= 3 and np.array_equal(_bits(got[0]), _bits(want[0]))
    assert all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))


# ---- 6. sharded ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_selection_over_a_3pt_batch(mh, engine):
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "propose_3pt_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)          # a stranded rank would run into these
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda d: d["rank"])
    assert [d["rank"] for d in recs] == [0, 1]
    # the single-rank calls over the same 600 hypotheses
    sc = _scene(mh)
    engine.set_params(2.6, 2.5, 0.005, 0.5, 20)
    _load(engine, sc)
    for name, refit in (("p3", 0), ("p3_refit", 1), ("p3_again", 0)):
        engine.set_tuning(30, refit)
        engine.propose_3pt(SEED, 0, 600)
        H, counters, counts, _ = engine.select_greedy(THR2, NEED, MAX_MODELS, np.ones(sc.n, np.uint8))
        assert len(counters) >= 3
        for rr in recs:
            assert rr[name]["ok"], rr[name]
            assert rr[name]["counters"] == counters.tolist() and rr[name]["counts"] == counts.tolist(), name
            assert rr[name]["H"] == H.view(np.uint64).tolist(), name
    for rr in recs:
        assert not rr["mixed"]["ok"] and rr["mixed"]["code"] == INVALID and "same residual mode" in rr["mixed"]["msg"], rr["mixed"]
        assert "mh_propose_3pt" in rr["mixed"]["msg"]
    # the host class with one hypothesis for two ranks (rank 1's shard is empty): the unsharded result on both ranks
    for rr in recs:
        assert rr["class_unsharded"]["k"] >= 0, rr["class_unsharded"]["k"]
        assert rr["class_empty_shard"] == rr["class_unsharded"] == recs[0]["class_unsharded"]


# ---- 7. the host class --------------------------------------------------------------------------------------------------------
def _run_process(host, sc, seed=5, hypotheses=4000, max_models=16, iter_hypotheses=0):
    dp = C.POINTER(C.c_double)
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((64, 9))
    it, en = C.c_int(-1), C.c_double(-1)
    src, dst, aff, F, e2 = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff, sc.F, sc.e2))
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, F.ctypes.data_as(dp),
                             e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.5), C.c_double(0.005), C.c_double(0.5), 20,
                             C.c_ulonglong(seed), hypotheses, max_models, 0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 64, C.byref(it), C.byref(en), None, iter_hypotheses, 4)
    C.CDLL(None).fflush(None)
    return k, labels, Hout[:max(k, 0)].copy()


def test_process_with_3pt_proposals(mh, engine_lib, capfd, monkeypatch):
    monkeypatch.setenv("MULTIH_TIMING", "1")                      # the stage log, which names the initial batch
    sc = mh.synth.make_scene(2000, 5, seed=99)
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    default = _run_process(host, sc)
    assert "3PT hypotheses" not in capfd.readouterr().out
    planes_default = mh.synth.agreement(sc.gt_label, default[1])["planes_recovered"]
    try:
        host.mhh_set_proposal_source(2, 0, 1)
        for iter_hypotheses in (0, 1000):                          # the initial batch alone; the iterative batches too
            k, labels, H = _run_process(host, sc, iter_hypotheses=iter_hypotheses)
            log = capfd.readouterr().out
            assert k >= 2 and labels.min() >= -1 and labels.max() < k
            got = mh.synth.agreement(sc.gt_label, labels)
            with capfd.disabled():
                print(f"3PT, iterative {iter_hypotheses}: {k} models, planes {got['planes_recovered']} of {got['planes']} "
                      f"(default route {planes_default}), ARI {got['ari']:.4f}")
            assert "models from 4000 3PT hypotheses" in log, log[-1500:]
            if iter_hypotheses == 0:
                assert got["planes_recovered"] >= planes_default
    finally:
        host.mhh_set_proposal_source(0, 16, 1)
    # the source is not sticky on a pooled engine: the default route is what it was
    again = _run_process(host, sc)
    assert "3PT hypotheses" not in capfd.readouterr().out
    assert again[0] == default[0] and np.array_equal(again[1], default[1])
    assert np.array_equal(again[2].view(np.uint64), default[2].view(np.uint64))


def test_harness_points_route_with_3pt_proposals(mh, engine_lib, tmp_path):
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    sc = mh.synth.make_scene(5000, 4, with_neighbours=False)
    corr = tmp_path / "corr.txt"
    np.savetxt(corr, np.concatenate([sc.src, sc.dst], axis=1), fmt="%.17g")
    planes = {}
    for name, extra in (("points", ["--points"]), ("3pt", ["--points", "--proposals", "3pt"])):
        out = tmp_path / f"{name}.out"
        r = subprocess.run([harness, str(corr), str(out), *extra], capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, MULTIH_TIMING="1"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        res = np.loadtxt(out, ndmin=2)
        assert res.shape[1] == 5
        full = np.full(sc.n, -1, dtype=np.int64)
        if res.shape[0] == sc.n:
            full[:] = res[:, 4]
        else:                                                      # the kept rows, taken back to their input rows (test_gpu_points_only.py)
            for a in range(0, res.shape[0], 512):
                d = ((res[a:a + 512, None, :2] - sc.src[None, :, :]) ** 2).sum(-1)
                full[np.argmin(d, axis=1)] = res[a:a + 512, 4]
        got = mh.synth.agreement(sc.gt_label, full)
        planes[name] = got["planes_recovered"]
        print(f"--{' '.join(extra)}: planes {got['planes_recovered']} of {got['planes']}, ARI {got['ari']:.4f}")
        assert ("3PT hypotheses" in r.stdout) == (name == "3pt")
    assert planes["3pt"] >= planes["points"]
