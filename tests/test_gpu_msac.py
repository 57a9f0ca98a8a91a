"""GPU tests of the MSAC-weighted score (mh_score_msac, mh_select_best_msac; include/multih_hip.h) against the numpy twin of
tests/msac_numpy.py, which tests/test_msac_cpu.py pins to the oracle's counts and to known answers.  Every comparison is exact
integer equality.

Both forms — k_msac32 behind the FP32 pre-test and k_msac64 (mh_set_tuning key 15 = 0, or inputs the pre-test is not proved
for) — at the sizes where a kernel takes another path: lane groups of 4, the 1 024-point tile and its tail, the 64-model block,
more than one block; on models that make d2 = 0, a non-finite d2, d2 within a few ulp of thr2 on either side, and far pairs."""
import ctypes as C
import os

import numpy as np
import pytest

import msac_numpy as W

pytestmark = pytest.mark.gpu
THR, LOCALITY = 2.2, 0.005
THR2 = THR * THR
NS = (1, 3, 255, 1024, 1025, 4099)
MS = (1, 63, 64, 65, 129)
K_SCORE = 2


def _near_thr2_offsets():
    """Offsets dx with fl(dx * dx) within a few ulp of thr2, on both sides of it."""
    dx = [np.sqrt(THR2)]
    for _ in range(4):
        dx.insert(0, np.nextafter(dx[0], 0.0))
        dx.append(np.nextafter(dx[-1], np.inf))
    return np.array(dx)


@pytest.fixture(scope="module")
def pool(synth, oracle):
    """4 099 points and 129 models, and the forward error of every pair (the oracle's, bit-equal to the engine's), once."""
    sc = synth.make_scene(4099, 3, seed=5, with_neighbours=False)
    src, dst = sc.src.copy(), sc.dst.copy()
    dx = _near_thr2_offsets()
    # against the identity (model 0): src = (0, 0), dst = (dx, 0) or (0, dx) -> d2 = fl(dx * dx) exactly; the point (2, 1)
    # makes s = 0 for models 1 (d2 = inf) and 2 (0 / 0: d2 = NaN)
    special = [((0.0, 0.0), (dx[3], 0.0)), ((2.0, 1.0), (5.0, 7.0)), ((0.0, 0.0), (0.0, dx[5]))]
    special += [((0.0, 0.0), (v, 0.0)) for v in dx] + [((0.0, 0.0), (0.0, 0.0)), ((2.0, 1.0), (2.0, 1.0))]
    for at in (0, 1018, 4099 - len(special)):                   # the first points (n = 1, 3), across the tile edge, the tail
        for j, (s, d) in enumerate(special):
            src[at + j], dst[at + j] = s, d
    rng = np.random.default_rng(5)
    H = [np.eye(3).reshape(9), np.array([1, 0, 0, 0, 1, 0, -0.5, 0, 1.0]), np.array([1, 0, -2.0, 0, 1, 0, -0.5, 0, 1.0])]
    H += list(sc.H_true)
    while len(H) < 129:
        if len(H) % 2:
            H.append(sc.H_true[len(H) % 3] * (1.0 + rng.normal(0, 1e-3, size=9)))       # near a plane: many pairs inside thr2
        else:
            H.append((np.eye(3) + rng.normal(0, 0.05, size=(3, 3))).reshape(9))          # far from everything
    H = np.ascontiguousarray(np.array(H))
    with np.errstate(all="ignore"):
        d2 = oracle.residual_matrix(src, dst, H)
    ulp = np.spacing(THR2)
    row = d2[0]
    assert ((row < THR2) & (THR2 - row <= 8 * ulp)).any() and ((row >= THR2) & (row - THR2 <= 8 * ulp)).any(), "near-miss pairs on both sides of thr2"
    assert (row == 0.0).any() and np.isinf(d2[1]).any() and np.isnan(d2[2]).any()
    assert (d2[3:] < THR2).mean() > 0.02 and (d2[3:] > 100 * THR2).mean() > 0.2
    mask = (rng.random(4099) < 0.7).astype(np.uint8)
    mask[[0, 2, 1020, 1024, 4098]] = 0
    mask[[1, 1019, 1023, 1025, 4097]] = 1
    return src, dst, H, d2, mask


_hip = None


def _read_ints(engine, which, count):
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    ptr, nbytes = engine.device_buffer(which)
    assert nbytes == 4 * count
    out = np.empty(count, dtype=np.int32)
    engine.synchronize()
    assert _hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), 4 * count, 2) == 0      # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("form", ["pretest", "fp64"])
def test_both_forms_equal_the_twin(mh, engine, pool, form, masked):
    src, dst, H, d2, mask = pool
    if form == "fp64":
        engine.set_tuning(15, 0)
    for n in NS:
        engine.set_correspondences(src[:n], dst[:n])
        mk = mask[:n] if masked else None
        for m in MS:
            engine.set_models(H[:m])
            want_c, want_w = W.sums_of_d2(d2[:m, :n], THR2, mk)
            cnt, wgt = engine.score_msac(THR2, mk)
            where = (form, masked, n, m)
            assert np.array_equal(cnt, want_c), where
            assert np.array_equal(wgt, want_w), where
            assert np.array_equal(_read_ints(engine, mh.capi.BUF_WEIGHTS, m), wgt), where
            assert np.array_equal(_read_ints(engine, mh.capi.BUF_COUNTS, m), cnt), where
            assert np.array_equal(engine.score(THR2, mk), want_c), where
    assert want_w.max() > 256 * 100 and (want_w <= 256 * want_c).all() and (want_w < 256 * want_c).any()


@pytest.mark.parametrize("form", ["pretest", "fp64"])
def test_halves_round_away_from_zero(engine, form):
    """d2 / thr2 = 507 / 512 exactly and 256 (1 - q) = 2.5: the weight is 3 (half-to-even would give 2)."""
    if form == "fp64":
        engine.set_tuning(15, 0)
    engine.set_correspondences(np.array([[0.0, 0.0]]), np.array([[507.0, 0.0]]))
    engine.set_models(np.eye(3).reshape(1, 9))
    cnt, wgt = engine.score_msac(259584.0)
    assert cnt.tolist() == [1] and wgt.tolist() == [3]


def test_inputs_outside_the_pretest_take_the_plain_form(engine, pool):
    src, dst, H, d2, mask = pool
    n, m = 1025, 65
    # thr2 outside [2^-40, 2^40]
    engine.set_correspondences(src[:n], dst[:n])                 # (a new point count empties the model set: points first)
    engine.set_models(H[:m])
    for thr2 in (2.0 ** -41, 2.0 ** 41):
        before = engine.score_stats()
        cnt, wgt = engine.score_msac(thr2)
        want_c, want_w = W.sums_of_d2(d2[:m, :n], thr2)
        assert np.array_equal(cnt, want_c) and np.array_equal(wgt, want_w), thr2
        after = engine.score_stats()
        assert after[0] - before[0] == n * m and after[1] - before[1] == n * m, "every pair through the FP64 formula"
    assert want_c.max() > 100
    # one coordinate at 2^20
    src2, dst2 = src[:n].copy(), dst[:n].copy()
    src2[7] = (2.0 ** 20, 3.0)
    dst2[7] = (2.0 ** 20 + 1.0, 3.0)
    engine.set_correspondences(src2, dst2)
    engine.set_models(H[:m])
    want_c, want_w = W.score_msac(src2, dst2, H[:m], THR2, mask[:n])
    cnt, wgt = engine.score_msac(THR2, mask[:n])
    assert np.array_equal(cnt, want_c) and np.array_equal(wgt, want_w)
    assert want_c[0] > 0 and want_w.max() > 0


def test_errors(mh, engine, pool):
    src, dst, H, _, _ = pool
    lib, h = engine.lib, engine._h
    engine.set_correspondences(src[:300], dst[:300])
    engine.set_models(H[:5])
    idx, w, c = C.c_longlong(0), C.c_int(0), C.c_int(0)
    assert lib.mh_select_best_msac(h, C.byref(idx), C.byref(w), C.byref(c)) == -4, "no weights yet"
    engine.set_residual_mode(True)
    assert lib.mh_score_msac(h, C.c_double(THR2), None, None, None) == -2
    assert b"forward" in lib.mh_last_error()
    engine.set_residual_mode(False)
    engine.score_msac(THR2)
    assert engine.select_best_msac()[0] >= 0
    for stale in ("set_models", "propose", "set_correspondences"):
        engine.score_msac(THR2)
        engine.select_best_msac()
        if stale == "set_models":
            engine.set_models(H[:5])
        elif stale == "propose":
            engine.propose_dlt4(3, 0, 5)
        else:
            engine.set_correspondences(src[:300], dst[:300])
        assert lib.mh_select_best_msac(h, C.byref(idx), C.byref(w), C.byref(c)) == -4, stale
        with pytest.raises(mh.MultiHError):
            engine.device_buffer(mh.capi.BUF_WEIGHTS)
    # n * 256 > INT32_MAX: refused before anything is launched
    n = 8388608
    big = np.zeros((n, 2))
    engine.set_correspondences(big, big)
    engine.set_models(H[:1])
    engine.profile_enable(True)
    engine.synchronize()
    launches = engine.profile_get(K_SCORE)[0]
    assert lib.mh_score_msac(h, C.c_double(THR2), None, None, None) == -5
    engine.synchronize()
    assert engine.profile_get(K_SCORE)[0] == launches
    engine.score(THR2, fetch=False)                              # (the counter does count)
    engine.synchronize()
    assert engine.profile_get(K_SCORE)[0] == launches + 1


@pytest.mark.parametrize("form", ["pretest", "fp64"])
def test_the_winner_by_weight_differs_from_the_winner_by_count(engine, form):
    """Model A (the identity) holds 10 points at d2 ~ 0.9 thr2, model B (a shift by 100) holds 5 points exactly."""
    if form == "fp64":
        engine.set_tuning(15, 0)
    rng = np.random.default_rng(3)
    src = np.floor(rng.uniform(0, 500, size=(15, 2)))
    dst = src.copy()
    dst[:10, 0] += np.sqrt(0.9 * THR2)
    dst[10:, 0] += 100.0
    A = np.eye(3).reshape(9)
    B = np.array([1, 0, 100.0, 0, 1, 0, 0, 0, 1.0])
    engine.set_correspondences(src, dst)
    engine.set_models(np.array([A, B, B]))
    cnt, wgt = engine.score_msac(THR2)
    want_c, want_w = W.score_msac(src, dst, np.array([A, B, B]), THR2)
    assert np.array_equal(cnt, want_c) and np.array_equal(wgt, want_w)
    assert cnt.tolist() == [10, 5, 5] and wgt[1] == wgt[2] == 1280 and 0 < wgt[0] < 1280
    assert engine.select_best() == (0, 10)                       # by count, from the counts mh_score_msac left resident
    assert engine.select_best_msac() == (1, 1280, 5)             # by weight; the duplicate at index 2 loses the tie
    engine.set_models(np.array([B, A, B]))
    engine.score_msac(THR2, fetch=False)
    assert engine.select_best_msac() == (0, 1280, 5)
    engine.select_best(fetch=False)                              # the counts buffer goes to an exchange: the winner's count survives
    assert engine.select_best_msac() == (0, 1280, 5)
    assert np.array_equal(engine.get_model(2), B) and np.array_equal(engine.get_model(1), A)


@pytest.mark.parametrize("form", ["pretest", "fp64"])
def test_mh_score_is_unchanged_and_the_statistics_grow(engine, pool, form):
    src, dst, H, d2, _ = pool
    if form == "fp64":
        engine.set_tuning(15, 0)
    n, m = 4099, 129
    engine.set_correspondences(src, dst)
    engine.set_models(H)
    before = engine.score(THR2)
    assert np.array_equal(before, (d2 < THR2).sum(axis=1))
    engine.score_stats(reset=True)
    for k in range(1, 3):
        cnt, _ = engine.score_msac(THR2)
        pairs, fp64 = engine.score_stats()
        assert pairs == k * n * m
        assert k * int(cnt.sum()) <= fp64 <= k * n * m
        if form == "fp64":
            assert fp64 == k * n * m
    assert np.array_equal(engine.score(THR2), before)
    assert engine.score_stats()[0] == 2 * n * m + (n * m if form == "pretest" else 0)


def _process(mh, sc, seed, hypotheses):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    dp = C.POINTER(C.c_double)
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((8, 9))
    src, dst, aff = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff))
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n,
                             None, None, C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5), 20,
                             C.c_ulonglong(seed), hypotheses, 8, 0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 8, None, None, None, 0, 4)
    return k, labels, Hout


def test_the_degenerate_tail_by_weight(mh, engine_lib, synth, oracle):
    """The single-plane scene of tests/test_gpu_parity.py::test_degenerate_tail_labels_the_original_points: Process() ends in
    HandleDegenerateCase, which under TAIL_SCORE_MSAC takes the hypothesis of the highest weight.  Expected from the twin: the
    tail's tuples and models are the oracle's (bit-equal to the engine's DLT), the weights the twin's."""
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_tail_score.argtypes = [C.c_int]
    host.mhh_set_tail_score.restype = None
    sc = synth.make_scene(3000, 1, seed=5, outlier_frac=0.35)
    seed, M = 99, 4000
    idx = oracle.sample4(seed ^ 0xdead, 0, M, sc.n)
    with np.errstate(all="ignore"):
        Hm, _, _ = oracle.dlt4(sc.src, sc.dst, idx)
        d2 = oracle.residual_matrix(sc.src, sc.dst, Hm)
    cnt, wgt = W.sums_of_d2(d2, THR2)
    by_weight, by_count = W.best_by_weight(wgt), int(np.argmax(cnt))
    host.mhh_set_tail_score(1)
    try:
        k, labels, Hout = _process(mh, sc, seed, M)
    finally:
        host.mhh_set_tail_score(-1)
    assert k == 1
    assert np.array_equal(labels, np.where(d2[by_weight] < THR2, 0, -1))
    assert np.array_equal(Hout[0].view(np.uint64), Hm[by_weight].view(np.uint64))
    with np.errstate(all="ignore"):
        assert np.array_equal(labels == 0, oracle.residual_matrix(sc.src, sc.dst, Hout[:1])[0] < THR2)
    # without the hook: the tail by count, as before
    k, labels, Hout = _process(mh, sc, seed, M)
    assert k == 1
    assert np.array_equal(labels, np.where(d2[by_count] < THR2, 0, -1))
    assert np.array_equal(Hout[0].view(np.uint64), Hm[by_count].view(np.uint64))
    assert (labels == 0).sum() > 0.5 * (sc.gt_label == 0).sum()
    host.mhh_set_tail_score(2)                                  # an unknown value: Process() fails with a message
    try:
        assert _process(mh, sc, seed, M)[0] == -1
    finally:
        host.mhh_set_tail_score(-1)
