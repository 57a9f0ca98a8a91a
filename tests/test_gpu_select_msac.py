"""GPU tests of the greedy selection — ranked by MSAC weight (mh_select_greedy_msac; include/multih_hip.h) and, through the same
round kernels, by count (mh_select_greedy) — against the numpy twin of tests/select_msac_numpy.py, which
tests/test_select_msac_cpu.py pins to the oracle's sequential selection and to known answers.  Positions, counts, weights (where
the entry point returns them) and masks are compared exactly, selected models bit for bit."""
import contextlib
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import select_msac_numpy as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR2 = 2.2 ** 2
NEED, MAX_MODELS = 20, 8
INVALID = -2


def _holes(n):
    m = np.ones(n, np.uint8)
    m[::7] = 0
    m[5:40] = 0
    return m


RANK_BY = ("count", "weight")


def _select(engine, rank_by, *args, **kw):
    """The mode's entry point, its outputs in the twin's order; mh_select_greedy returns no weights: None in their place."""
    if rank_by == "weight":
        return engine.select_greedy_msac(*args, **kw)
    H, counters, counts, mask = engine.select_greedy(*args, **kw)
    return H, counters, counts, None, mask


def _same(got, want, where):
    H, counters, counts, weights, mask = got
    H_t, idx_t, cnt_t, wgt_t, mask_t = want
    assert np.array_equal(counters, idx_t), where
    assert np.array_equal(counts, cnt_t) and (weights is None or np.array_equal(weights, wgt_t)), where
    assert np.array_equal(mask, mask_t), where
    assert np.array_equal(H.view(np.uint64), H_t.view(np.uint64)), where


_twin = {}


def _case(mh, engine, n, M, holes, rank_by="weight"):
    """Loads scene n and batch M into the engine; returns (mask, the twin's selection) — the twin runs once per case."""
    sc = mh.synth.make_scene(n, 2 if n < 1000 else 3, seed=n, with_neighbours=False)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.propose_dlt4(n + M, 0, M)
    mask = _holes(n) if holes else np.ones(n, np.uint8)
    key = (n, M, holes, rank_by)
    if key not in _twin:
        _twin[key] = T.select_greedy(sc.src, sc.dst, engine.get_models(), THR2, NEED, MAX_MODELS, mask, rank_by=rank_by)
    return mask, _twin[key]


def _parity(mh, engine, rank_by, key36, key15, holes):
    engine.set_tuning(36, key36)
    engine.set_tuning(15, key15)
    rounds = 0
    for n in (257, 1000, 4099):
        for M in (300, 3001):
            mask, want = _case(mh, engine, n, M, holes, rank_by)
            got = _select(engine, rank_by, THR2, NEED, MAX_MODELS, mask)
            _same(got, want, (rank_by, key36, key15, holes, n, M))
            assert np.array_equal(got[0].view(np.uint64), engine.get_models()[got[1]].view(np.uint64)), "H_out: the batch's rows"
            # without a mask: all points
            if not holes:
                H2, c2, n2, w2, m2 = _select(engine, rank_by, THR2, NEED, MAX_MODELS)
                assert m2 is None and np.array_equal(c2, want[1]) and np.array_equal(n2, want[2])
                assert w2 is None or np.array_equal(w2, want[3])
            rounds += len(got[1])
    assert rounds >= 6 * 2, "the scenes must take several rounds"


def _grid(test):
    for name, values in (("key36", [1, 0]), ("key15", [1, 0]), ("holes", [False, True])):
        test = pytest.mark.parametrize(name, values)(test)
    return test


@_grid
def test_parity_with_the_twin(mh, engine, key36, key15, holes):
    _parity(mh, engine, "weight", key36, key15, holes)


@_grid
def test_parity_with_the_twin_by_count(mh, engine, key36, key15, holes):
    """The same shapes through mh_select_greedy.  At n = 4099 the two modes pick differently."""
    _parity(mh, engine, "count", key36, key15, holes)


@pytest.mark.parametrize("key36", [1, 0])
@pytest.mark.parametrize("rank_by", RANK_BY)
def test_batch_sizes_at_the_compaction_workgroup_edge(mh, engine, rank_by, key36):
    """One workgroup of the compaction holds 256 candidates: a batch one short of it, exactly it, one more."""
    engine.set_tuning(36, key36)
    for M in (255, 256, 257):
        mask, want = _case(mh, engine, 257, M, False, rank_by)
        _same(_select(engine, rank_by, THR2, NEED, MAX_MODELS, mask), want, (rank_by, key36, M))


def test_count_and_weight_differ_where_they_should(engine):
    src, dst, H = T.tight_and_sloppy(THR2)
    engine.set_correspondences(src, dst)
    for need, by_count, by_weight in ((20, [0, 1], [1, 0]), (35, [0], [0])):
        engine.set_models(H)
        _, idx_c, cnt_c, _ = engine.select_greedy(THR2, need, 8)
        assert idx_c.tolist() == by_count
        engine.set_models(H)
        got = engine.select_greedy_msac(THR2, need, 8, np.ones(70, np.uint8))
        assert got[1].tolist() == by_weight
        _same(got, T.select_greedy(src, dst, H, THR2, need, 8), need)
    assert got[2].tolist() == [40] and got[4].sum() == 30          # need = 35: the tight model is never eligible


@pytest.mark.parametrize("rank_by", RANK_BY)
def test_hand_built_sets_in_both_modes(engine, rank_by):
    """The eligibility rule at its edges: count == need is eligible, need - 1 is not; nobody eligible selects nothing and
    leaves the mask as it came; an empty support set; one model only; a tie; a winner of weight 0."""
    src, dst, H = T.tight_and_sloppy(THR2)
    engine.set_correspondences(src, dst)
    ones = np.ones(70, np.uint8)

    def run(need, max_models=8, mask=None):
        mask = ones if mask is None else mask
        engine.set_models(H)
        got = _select(engine, rank_by, THR2, need, max_models, mask)
        _same(got, T.select_greedy(src, dst, H, THR2, need, max_models, mask, rank_by=rank_by), (rank_by, need, max_models))
        return got

    got = run(30)
    assert got[1].tolist() == ([0, 1] if rank_by == "count" else [1, 0])
    assert got[2].tolist() == ([40, 30] if rank_by == "count" else [30, 40])
    for need in (31, 40):
        got = run(need)
        assert got[1].tolist() == [0] and got[2].tolist() == [40] and got[4].sum() == 30
    got = run(41)
    assert len(got[1]) == 0 and got[0].shape == (0, 9) and np.array_equal(got[4], ones)
    assert run(20, max_models=1)[1].tolist() == ([0] if rank_by == "count" else [1])
    got = run(20, mask=np.zeros(70, np.uint8))
    assert len(got[1]) == 0 and not got[4].any()
    src, dst, H = T.tie(THR2)
    engine.set_correspondences(src, dst)
    ones = np.ones(40, np.uint8)
    assert run(NEED)[1].tolist() == [3]
    src, dst, H = T.weight_zero(THR2)
    engine.set_correspondences(src, dst)
    ones = np.ones(25, np.uint8)
    got = run(NEED)
    assert got[1].tolist() == [1] and got[2].tolist() == [25]


def test_ties_go_to_the_lowest_position(engine):
    src, dst, H = T.tie(THR2)
    engine.set_correspondences(src, dst)
    engine.set_models(H)
    got = engine.select_greedy_msac(THR2, NEED, 8, np.ones(40, np.uint8))
    assert got[1].tolist() == [3] and 7 not in got[1].tolist()
    _same(got, T.select_greedy(src, dst, H, THR2, NEED, 8), "tie")


def test_weight_zero_still_wins(engine):
    src, dst, H = T.weight_zero(THR2)
    want = T.select_greedy(src, dst, H, THR2, NEED, 8)
    assert want[1].tolist() == [1] and want[2].tolist() == [25] and want[3].tolist() == [0], "the twin computes the actual weight"
    engine.set_correspondences(src, dst)
    engine.set_models(H)
    _same(engine.select_greedy_msac(THR2, NEED, 8, np.ones(25, np.uint8)), want, "weight 0")


def _models_equal(a, b):
    """As test_greedy_selection_with_refitted_winners compares its models: bit for bit."""
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_refitted_winners(mh, engine):
    sc = mh.synth.make_scene(3000, 3, seed=5, with_neighbours=False)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_epipolar(sc.F, sc.e2)
    engine.propose_dlt4(9, 0, 2000)
    H = engine.get_models()
    plain = engine.select_greedy_msac(THR2, NEED, MAX_MODELS, np.ones(sc.n, np.uint8))
    engine.set_tuning(30, 1)
    for key36 in (1, 0):
        engine.set_tuning(36, key36)
        engine.propose_dlt4(9, 0, 2000)
        got = engine.select_greedy_msac(THR2, NEED, MAX_MODELS, np.ones(sc.n, np.uint8))
        want = T.select_greedy(sc.src, sc.dst, H, THR2, NEED, MAX_MODELS, refit=T.haf_refit(sc.src, sc.dst, sc.aff, sc.F, sc.e2))
        assert len(got[1]) >= 3
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
        assert np.array_equal(got[4], want[4])
        assert _models_equal(got[0], want[0])
    assert got[1][0] == plain[1][0] and got[3][0] == plain[3][0] and not np.array_equal(got[0][0], plain[0][0]), "the first winner is the same hypothesis, refitted"
    # a refit that is finite but lighter than its hypothesis: the hypothesis' H is kept (built and confirmed on the CPU:
    # tests/test_select_msac_cpu.py::test_a_finite_but_lighter_refit_is_not_taken)
    sc, H, e2 = T.lighter_refit_scene(mh.synth)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_epipolar(sc.F, e2)
    engine.set_models(H)
    got = engine.select_greedy_msac(THR2, NEED, MAX_MODELS, np.ones(sc.n, np.uint8))
    want = T.select_greedy(sc.src, sc.dst, H, THR2, NEED, MAX_MODELS, refit=T.haf_refit(sc.src, sc.dst, sc.aff, sc.F, e2))
    assert np.array_equal(want[0][0], H[want[1][0]])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert np.array_equal(got[4], want[4]) and _models_equal(got[0], want[0])
    # without the epipolar geometry the option is refused, not ignored
    e2_ = mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20)
    try:
        e2_.set_correspondences(sc.src, sc.dst, sc.aff)
        e2_.set_models(H)
        e2_.set_tuning(30, 1)
        with pytest.raises(mh.MultiHError) as ei:
            e2_.select_greedy_msac(THR2, NEED, 4)
        assert ei.value.code == -4
    finally:
        e2_.close()


def test_refusals(mh, engine):
    sc = mh.synth.make_scene(1000, 3, seed=1000, with_neighbours=False)
    engine.set_correspondences(sc.src, sc.dst)
    engine.propose_dlt4(4, 0, 300)
    before = engine.select_greedy(THR2, NEED, MAX_MODELS, np.ones(sc.n, np.uint8))
    lib, h = engine.lib, engine._h
    Hout, k = np.zeros((8, 9)), C.c_int(-1)
    dp = Hout.ctypes.data_as(C.POINTER(C.c_double))

    def call(need=NEED, H_out=dp, n_models=8):
        return lib.mh_select_greedy_msac(h, C.c_double(THR2), need, n_models, None, H_out, None, None, None, C.byref(k), C.c_longlong(0))

    engine.set_residual_mode(True)
    assert call() == INVALID and b"forward" in lib.mh_last_error()
    engine.set_residual_mode(False)
    assert call(H_out=None) == INVALID
    assert call(need=0) == INVALID
    assert call(n_models=0) == INVALID
    assert lib.mh_select_greedy_msac(h, C.c_double(THR2), NEED, 8, None, dp, None, None, None, None, C.c_longlong(0)) == INVALID
    assert call() == 0 and k.value >= 2
    engine.propose_dlt4(4, 0, 300)
    after = engine.select_greedy(THR2, NEED, MAX_MODELS, np.ones(sc.n, np.uint8))
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    # 256 n > INT32_MAX: refused before anything is launched
    n = 8388608
    big = np.zeros((n, 2))
    engine.set_correspondences(big, big)
    engine.set_models(np.eye(3).reshape(1, 9))
    engine.profile_enable(True)
    engine.synchronize()
    launches = engine.profile_get(2)[0]
    assert call() == -5
    engine.synchronize()
    assert engine.profile_get(2)[0] == launches


@contextlib.contextmanager
def _one_rank_comm(mh, engine):
    """The pattern of tests/test_gpu_pipeline.py: RCCL's ncclAllGather on a one-rank communicator runs the whole protocol."""
    rl = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_rccl.so"))
    rl.mhr_last_error.restype = C.c_char_p
    rl.mhr_calls.restype = C.c_longlong
    uid = (C.c_ubyte * 128)()
    assert rl.mhr_unique_id(uid) == 0, rl.mhr_last_error()
    comm = C.c_void_p()
    assert rl.mhr_init(C.byref(comm), 0, 1, uid, 0) == 0, rl.mhr_last_error()
    try:
        yield rl, comm
    finally:
        engine.set_transport(0, 1)
        rl.mhr_destroy(comm)


def test_a_one_rank_transport_gives_the_unsharded_outputs(mh, engine):
    with _one_rank_comm(mh, engine) as (rl, comm):
        sc = mh.synth.make_scene(4000, 4, seed=31, with_neighbours=False)
        engine.set_correspondences(sc.src, sc.dst, sc.aff)
        engine.propose_dlt4(77, 0, 3001)
        ones = np.ones(sc.n, np.uint8)
        plain = engine.select_greedy_msac(THR2, NEED, MAX_MODELS, ones)
        engine.set_transport(0, 1, stream_fn=rl.mhr_allgather, ctx=comm)
        calls = rl.mhr_calls(comm)
        via = engine.select_greedy_msac(THR2, NEED, MAX_MODELS, ones, total_m=3001)
        used = rl.mhr_calls(comm) - calls
        for a, b in zip(plain, via):
            assert np.array_equal(a, b)
        assert len(plain[1]) >= 4
        rounds = len(via[1]) + (1 if len(via[1]) < MAX_MODELS else 0)
        assert used == rounds + 1, "one record per round and the first round's score vector: mh_select_greedy's collectives"


@pytest.mark.parametrize("rank_by", RANK_BY)
def test_nobody_eligible_behind_a_transport(mh, engine, rank_by):
    """No candidate reaches `need`: no key on any rank, -1 throughout the gathered vector; zero models and no error."""
    src, dst, H = T.tight_and_sloppy(THR2)
    ones = np.ones(70, np.uint8)
    with _one_rank_comm(mh, engine) as (rl, comm):
        engine.set_correspondences(src, dst)
        engine.set_models(H)
        engine.set_transport(0, 1, stream_fn=rl.mhr_allgather, ctx=comm)
        calls = rl.mhr_calls(comm)
        got = _select(engine, rank_by, THR2, 41, 8, ones, total_m=2)
        assert rl.mhr_calls(comm) - calls == 2, "the first round's score vector and its record"
        assert len(got[1]) == 0 and np.array_equal(got[4], ones)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_equal_one_and_mixed_entry_points_leave_together(mh, engine):
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "select_msac_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)          # a stranded rank would run into these
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda d: d["rank"])
    assert [d["rank"] for d in recs] == [0, 1]
    sc = mh.synth.make_scene(3000, 3, seed=3, with_neighbours=False)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.propose_dlt4(77, 0, 3001)
    H, counters, counts, weights, mask = engine.select_greedy_msac(THR2, NEED, MAX_MODELS, np.ones(sc.n, np.uint8))
    assert len(counters) >= 3
    for name in ("msac", "msac_again"):
        for rr in recs:
            assert rr[name]["ok"], rr[name]
            assert rr[name]["counters"] == counters.tolist() and rr[name]["counts"] == counts.tolist(), name
            assert rr[name]["weights"] == weights.tolist() and rr[name]["left"] == int(mask.sum()), name
            assert rr[name]["H"] == H.view(np.uint64).tolist(), name
    for rr in recs:
        assert not rr["mixed"]["ok"] and rr["mixed"]["code"] == INVALID and "mh_select_greedy_msac" in rr["mixed"]["msg"], rr["mixed"]


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


def test_the_class_in_either_mode(mh, engine_lib):
    """The small class scene of tests/test_gpu_local_sampler.py through mhh_run_process: the count mode set explicitly is the
    default bit for bit; the MSAC mode runs and returns valid labels (no plane-count or ARI floor: nobody has measured one)."""
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_selection_score.argtypes = [C.c_int]
    host.mhh_set_selection_score.restype = None
    sc = mh.synth.make_scene(2000, 3, seed=9)
    k0, lab0, H0 = _run_process(mh, sc)
    assert k0 >= 2
    try:
        host.mhh_set_selection_score(0)
        k1, lab1, H1 = _run_process(mh, sc)
        assert k1 == k0 and np.array_equal(lab1, lab0) and np.array_equal(H1.view(np.uint64), H0.view(np.uint64))
        host.mhh_set_selection_score(1)
        k2, lab2, H2 = _run_process(mh, sc)
        assert k2 >= 1 and lab2.min() >= -1 and lab2.max() == k2 - 1 and np.isfinite(H2).all()
        host.mhh_set_selection_score(2)                            # an unknown value: Process() fails with a message
        assert _run_process(mh, sc)[0] == -1
    finally:
        host.mhh_set_selection_score(-1)
    k3, lab3, _ = _run_process(mh, sc)
    assert k3 == k0 and np.array_equal(lab3, lab0)
