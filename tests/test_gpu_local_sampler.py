"""The neighbourhood-guided proposal sampler (mh_set_sampler, mh_build_sample_neighbours; csrc/dlt4.hip, sample4_by) on the
GPU: its table against brute force, its tuples against the numpy twin (tests/local_sampler_numpy.py) exactly, its models
against the oracle's DLT, the three forms of the proposer against each other, the sharded selection, and the host class."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import local_sampler_numpy as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

THR2 = 2.2 ** 2
UNIFORM, LOCAL = 0, 1
INVALID, NOT_SET = -2, -4
WRAP_FIRST, WRAP_SEED = (1 << 56) - 2, 1000        # (c << 8) passes 2^64 inside the batch, and seed + (c << 8) just before it
_scenes = {}


def _scene(mh, n):
    if n not in _scenes:
        _scenes[n] = mh.synth.make_scene(n, 3 if n >= 64 else 1, seed=5, with_neighbours=False)
    return _scenes[n]


def _load(engine, sc):
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_epipolar(sc.F, sc.e2)


def _code(mh, fn):
    with pytest.raises(mh.MultiHError) as ei:
        fn()
    return ei.value.code


# ---- 1. the table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(300, 3), (300, 8), (300, 32), (33, 32)])
@pytest.mark.parametrize("grid", [1, 0])
def test_table_equals_brute_force(mh, engine, n, k, grid):
    sc = _scene(mh, n)
    _load(engine, sc)
    engine.set_tuning(31, grid)
    engine.build_sample_neighbours(k)
    got = engine.get_sample_neighbours()
    assert got.shape == (n, k)
    assert np.array_equal(got, twin.knn_table(sc.src, sc.dst, k))


def test_table_leaves_the_labeling_graph_alone(mh, engine):
    sc = _scene(mh, 300)
    _load(engine, sc)
    assert _code(mh, engine.get_sample_neighbours) == NOT_SET
    engine.build_neighbors_knn(16)
    before = [a.copy() for a in engine.get_sym_graph()]
    engine.build_sample_neighbours(8)
    after = engine.get_sym_graph()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # ... and the other way round: a new labeling graph does not move the table
    tbl = engine.get_sample_neighbours()
    engine.build_neighbors_knn(5)
    assert np.array_equal(engine.get_sample_neighbours(), tbl)


def test_table_arguments_and_lifetime(mh, engine):
    sc = _scene(mh, 33)
    _load(engine, sc)
    for k in (2, 33):                                       # below 3; k = n (33 points)
        assert _code(mh, lambda: engine.build_sample_neighbours(k)) == INVALID
    big = _scene(mh, 300)
    _load(engine, big)
    assert _code(mh, lambda: engine.build_sample_neighbours(33)) == INVALID      # above 32 with k < n: that bound on its own
    engine.build_sample_neighbours(32)
    _load(engine, sc)
    engine.build_sample_neighbours(32)                      # k = n - 1 is the largest table of 33 points
    _load(engine, sc)                                       # (drops that table again)
    for bad in ((2, 0), (-1, 0), (LOCAL, 17), (LOCAL, -1)):
        assert _code(mh, lambda: engine.set_sampler(*bad)) == INVALID
    engine.set_sampler(LOCAL, 0)
    assert _code(mh, lambda: engine.propose_dlt4(1, 0, 10)) == NOT_SET
    assert _code(mh, lambda: engine.prefetch_dlt4(1, 0, 10)) == NOT_SET
    engine.build_sample_neighbours(8)
    engine.propose_dlt4(1, 0, 10)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)      # drops the table; the sampler setting stays
    assert _code(mh, lambda: engine.propose_dlt4(1, 0, 10)) == NOT_SET
    assert _code(mh, engine.get_sample_neighbours) == NOT_SET
    engine.set_sampler(UNIFORM, 0)
    engine.propose_dlt4(1, 0, 10)


# ---- 2. the tuples, exactly ---------------------------------------------------------------------------------------------
MS = (1, 15, 16, 17, 63, 64, 65, 1000)
FIRSTS = ((99, 0), (99, 10), (99, (1 << 40) + 5), (WRAP_SEED, WRAP_FIRST))      # (seed, first)


@pytest.mark.parametrize("n,k", [(4, 3), (64, 3), (64, 8), (64, 32), (300, 3), (300, 8), (300, 32)])
def test_tuples_equal_the_twin(mh, engine, oracle, n, k):
    sc = _scene(mh, n)
    _load(engine, sc)
    engine.build_sample_neighbours(k)
    nbr = twin.knn_table(sc.src, sc.dst, k)
    assert np.array_equal(engine.get_sample_neighbours(), nbr)
    for seed, first in FIRSTS:
        for u in (0, 4, 16):
            want = twin.sample_local(seed, first, max(MS), n, nbr, u)             # the tuple of a counter does not depend on m
            if u == 16:
                assert np.array_equal(want, oracle.sample4(seed, first, max(MS), n))
            for m in MS:
                engine.set_sampler(LOCAL, u)
                engine.propose_dlt4(seed, first, m)
                idx = engine.get_samples()
                assert np.array_equal(idx, want[:m]), (seed, first, u, m)
                if u == 16 and m in (17, 1000):
                    H = engine.get_models()
                    engine.set_sampler(UNIFORM, 0)
                    engine.propose_dlt4(seed, first, m)
                    assert np.array_equal(engine.get_samples(), idx)
                    assert np.array_equal(engine.get_models().view(np.uint64), H.view(np.uint64))


# ---- 3. the models ------------------------------------------------------------------------------------------------------
def test_models_equal_the_oracle_dlt(mh, engine, oracle):
    sc = mh.synth.make_scene(300, 3, seed=5)
    _load(engine, sc)
    engine.build_sample_neighbours(8)
    engine.set_sampler(LOCAL, 0)
    m = 1000
    engine.propose_dlt4(5, 10, m)
    idx = engine.get_samples()
    assert np.array_equal(idx, twin.sample_local(5, 10, m, sc.n, twin.knn_table(sc.src, sc.dst, 8), 0))
    H = engine.get_models()
    H_ref, wit, _ = oracle.dlt4(sc.src, sc.dst, idx)
    good = wit > 1e-6                         # conditioning witness, as test_sampling_and_dlt4 (the oracle keeps all 1000 here)
    print(f"kept {int(good.sum())} of {m}; max abs difference {np.max(np.abs(H[good] - H_ref[good])):.3e}")
    assert good.sum() > 0.5 * m
    assert np.max(np.abs(H[good] - H_ref[good])) <= 1e-6
    assert np.array_equal(H[good].view(np.uint64), H_ref[good].view(np.uint64))


# ---- 4. the forms -------------------------------------------------------------------------------------------------------
def test_register_lds_and_prefetched_forms_agree(mh, engine):
    sc = mh.synth.make_scene(3000, 3, seed=12, with_neighbours=False)
    _load(engine, sc)
    engine.build_sample_neighbours(16)
    engine.set_sampler(LOCAL, 4)
    nbr = engine.get_sample_neighbours()
    sizes = (700, 512, 1300, 90, 333)
    want = []
    try:
        for i, m in enumerate(sizes):
            per_form = []
            for form in (2, 1):                                   # registers, LDS
                engine.set_tuning(25, form)
                engine.propose_dlt4(33, 10000 * i, m)
                per_form.append((engine.get_samples(), engine.get_models()))
            assert np.array_equal(per_form[0][0], per_form[1][0]), i
            assert np.array_equal(per_form[0][1].view(np.uint64), per_form[1][1].view(np.uint64)), i
            want.append(per_form[0])
    finally:
        engine.set_tuning(25, 0)
    assert np.array_equal(want[3][0], twin.sample_local(33, 30000, sizes[3], sc.n, nbr, 4))
    # two batches ahead, changing sizes, sweeps in between (as test_two_batches_prefetched_ahead for the uniform sampler)
    engine.prefetch_dlt4(33, 0, sizes[0])
    engine.prefetch_dlt4(33, 10000, sizes[1])
    for i, m in enumerate(sizes):
        engine.adopt_prefetched()
        if i + 2 < len(sizes):
            engine.prefetch_dlt4(33, 10000 * (i + 2), sizes[i + 2])
        engine.residual_matrix(THR2, fetch_R=False)
        idx, H = engine.get_samples(), engine.get_models()
        assert np.array_equal(idx, want[i][0]) and np.array_equal(H.view(np.uint64), want[i][1].view(np.uint64)), i


# ---- 5. sticky and harmless ---------------------------------------------------------------------------------------------
def test_back_to_uniform_and_scores(mh, engine, oracle):
    sc = _scene(mh, 300)
    _load(engine, sc)
    engine.build_sample_neighbours(8)
    engine.set_sampler(LOCAL, 0)
    engine.propose_dlt4(7, 3, 500)
    loc = engine.get_samples()
    assert not np.array_equal(loc, oracle.sample4(7, 3, 500, sc.n))
    H = engine.get_models()
    assert np.array_equal(engine.score(THR2), oracle.score(sc.src, sc.dst, H, THR2))
    engine.set_sampler(UNIFORM, 0)
    engine.propose_dlt4(7, 3, 500)
    assert np.array_equal(engine.get_samples(), oracle.sample4(7, 3, 500, sc.n))


# ---- 6. sharded ---------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_selection_over_a_local_batch(mh, engine):
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "local_sampler_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)          # a stranded rank would run into these
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda d: d["rank"])
    assert [d["rank"] for d in recs] == [0, 1]
    r0, r1 = recs
    # the single-rank call over the same 3 000 hypotheses
    sc = mh.synth.make_scene(3000, 3, seed=3, with_neighbours=False)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.build_sample_neighbours(16)
    engine.set_sampler(LOCAL, 4)
    engine.propose_dlt4(77, 0, 3000)
    H, counters, counts, _ = engine.select_greedy(THR2, 20, 8, np.ones(sc.n, np.uint8))
    assert len(counters) >= 3
    for name in ("local", "local_again"):
        for rr in (r0, r1):
            assert rr[name]["ok"], rr[name]
            assert rr[name]["counters"] == counters.tolist() and rr[name]["counts"] == counts.tolist(), name
            assert rr[name]["H"] == H.view(np.uint64).tolist(), name
    for name in ("mixed", "other_share"):
        for rr in (r0, r1):
            assert not rr[name]["ok"] and rr[name]["code"] == INVALID and "same residual mode" in rr[name]["msg"], rr[name]
            assert "mh_set_sampler" in rr[name]["msg"]


# ---- 7. the host class --------------------------------------------------------------------------------------------------
def _run_process(mh, sc, seed=5, hypotheses=4000, max_models=16):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    dp = C.POINTER(C.c_double)
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((64, 9))
    it, en = C.c_int(-1), C.c_double(-1)
    src, dst, aff, F, e2 = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff, sc.F, sc.e2))
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, F.ctypes.data_as(dp),
                             e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5), 20,
                             C.c_ulonglong(seed), hypotheses, max_models, 0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 64, C.byref(it), C.byref(en), None, 0, 4)
    return k, labels, Hout[:max(k, 0)].copy()


@pytest.fixture(scope="module")
def class_scene_and_default_run(mh, engine_lib):
    """Process() by the default route BEFORE this file has called the sampler hook."""
    sc = mh.synth.make_scene(2000, 3, seed=9)
    return sc, _run_process(mh, sc)


def test_process_with_the_local_sampler(mh, class_scene_and_default_run):
    sc, default = class_scene_and_default_run
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    try:
        host.mhh_set_proposal_sampler(1, 32, 4)
        runs = [_run_process(mh, sc) for _ in range(2)]
    finally:
        host.mhh_set_proposal_sampler(0, 0, 0)
    k, labels, H = runs[0]
    assert k >= 2
    assert labels.min() >= -1 and labels.max() < k
    assert runs[1][0] == k and np.array_equal(runs[1][1], labels) and np.array_equal(runs[1][2].view(np.uint64), H.view(np.uint64))
    # the hook reset: the default route is what it was before any sampler hook was called
    again = _run_process(mh, sc)
    assert again[0] == default[0] and np.array_equal(again[1], default[1])
    assert np.array_equal(again[2].view(np.uint64), default[2].view(np.uint64))
    assert default[0] >= 2
