"""GPU tests of the minimal-sample F estimator: k_fund7 (7-point samples, up to three F each), the reuse of the Sampson /
point-to-line scoring on its 3 m slots, the device-side stop rule k_ransac_stop, mh_estimate_fundamental_minimal and the
host route (MultiH::SetFundamentalEstimator).  The yardstick is tests/fund7_numpy.py (LAPACK null space, np.roots), pinned
on the CPU by tests/test_fund7_reference.py; solutions are compared as sets of F per sample, never by null vector or root."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fund7_numpy as T

pytestmark = pytest.mark.gpu

MH_ERR_INVALID = -2


@functools.lru_cache(maxsize=None)
def _scene(n, noise=0.5):
    src, dst = T.make_scene(n, seed=101 + n, noise=noise)
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst


def _propose(engine, seed, first, m):
    engine.propose_fund7(seed, first, m)
    F = engine.get_fund7_hypotheses()
    idx, nvalid = engine.get_fund7_samples()
    return F, idx, nvalid


def _check_slots(F, nvalid):
    """Every slot all-NaN or all finite, the NaN ones trailing, nvalid = the finite ones."""
    finite = np.isfinite(F).all(axis=2)
    assert np.array_equal(np.isnan(F).all(axis=2), ~finite), "a slot is neither all-NaN nor finite"
    assert np.array_equal(finite.sum(axis=1), nvalid)
    assert np.array_equal(finite, np.arange(3)[None, :] < nvalid[:, None]), "a NaN slot in front of a finite one"
    return finite


# ---- shape edges of the kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 15, 16, 17, 63, 64, 65])
def test_shape_edges(engine, m):
    n = 64
    src, dst = _scene(n)
    engine.set_correspondences(src, dst)
    F, idx, nvalid = _propose(engine, 11, 0, m)
    assert F.shape == (m, 3, 9) and idx.shape == (m, 7) and nvalid.shape == (m,)
    _check_slots(F, nvalid)
    assert np.all((nvalid >= 0) & (nvalid <= 3))
    assert np.all((idx >= 0) & (idx < n)) and all(len(set(r)) == 7 for r in idx.tolist())
    assert np.array_equal(idx, T.sample7(11, 0, m, n))
    counts = engine.score_sampson(4.0)
    assert counts.shape == (3 * m,) and np.all((counts >= 0) & (counts <= n))


def test_offset_and_determinism(engine):
    src, dst = _scene(64)
    engine.set_correspondences(src, dst)
    F8, idx8, nv8 = _propose(engine, 21, 0, 8)
    F3, idx3, nv3 = _propose(engine, 21, 5, 3)
    assert np.array_equal(F3.view(np.uint64), F8[5:8].view(np.uint64))
    assert np.array_equal(idx3, idx8[5:8]) and np.array_equal(nv3, nv8[5:8])
    Fa, idxa, nva = _propose(engine, 21, 0, 8)
    assert np.array_equal(Fa.view(np.uint64), F8.view(np.uint64)) and np.array_equal(idxa, idx8) and np.array_equal(nva, nv8)


# ---- solutions against the twin --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 8, 64])
def test_solutions_match_the_twin(engine, n):
    """For every sample whose reference cubic has scaled root gap >= 1e-3: as many finite slots as the twin has real roots,
    every one within 1e-6 (Frobenius; unit-norm F) of a twin solution, unit norm, F[8] >= 0, |det F| and the seven
    |p2^T F p1| <= 1e-9.  At most 1 % of a case may be skipped."""
    m = 65
    src, dst = _scene(n)
    engine.set_correspondences(src, dst)
    F, idx, nvalid = _propose(engine, 11, 0, m)
    _check_slots(F, nvalid)
    skipped = 0
    worst_match = worst_res = worst_norm = 0.0
    first_set = None
    for s in range(m):
        ref, gap = T.solve7(src[idx[s]], dst[idx[s]])
        if gap < 1e-3:
            skipped += 1
            continue
        got = F[s, :nvalid[s]]
        assert nvalid[s] == len(ref), f"sample {s}: {nvalid[s]} finite slots, the twin has {len(ref)} real roots (gap {gap:.3g})"
        worst_match = max(worst_match, T.set_distance(got, ref))
        for f in got:
            det, res = T.constraint_residuals(f, src[idx[s]], dst[idx[s]])
            worst_res = max(worst_res, det, float(res.max()))
            worst_norm = max(worst_norm, abs(float(np.linalg.norm(f)) - 1.0))
            assert f[8] >= 0.0
        if n == 7:                       # every tuple is the same point set: the same solution set
            first_set = got if first_set is None else first_set
            assert len(got) == len(first_set)
            worst_match = max(worst_match, T.set_distance(got, first_set), T.set_distance(first_set, got))
    print(f"n={n}: worst distance to the twin {worst_match:.3g}, worst |det| / residual {worst_res:.3g}, "
          f"worst | |F| - 1 | {worst_norm:.3g}, skipped {skipped}/{m}")
    assert skipped <= m // 100, f"{skipped} of {m} samples skipped"
    assert worst_match <= 1e-6
    assert worst_norm <= 1e-12
    assert worst_res <= 1e-9


# ---- degenerate samples ------------------------------------------------------------------------------------------------------
def _degenerate(kind):
    src, dst = (a.copy() for a in _scene(7))
    if kind == "duplicate":
        src[3], dst[3] = src[1], dst[1]
    else:                                # all points on a line in both images
        t = np.linspace(0.0, 1.0, 7)
        src = np.stack([100.0 + 400.0 * t, 50.0 + 300.0 * t], axis=1)
        dst = np.stack([120.0 + 380.0 * t ** 1.5, 400.0 - 310.0 * t ** 1.5], axis=1)
    return src, dst


@pytest.mark.parametrize("kind", ["duplicate", "collinear"])
def test_degenerate_samples(engine, kind):
    src, dst = _degenerate(kind)
    engine.set_correspondences(src, dst)
    F, idx, nvalid = _propose(engine, 5, 0, 20)       # (status MH_OK: the binding raises otherwise)
    _check_slots(F, nvalid)
    for metric in (0, 1):
        engine.set_fundamental_metric(metric)
        counts = engine.score_sampson(4.0)
        assert np.all((counts >= 0) & (counts <= 7))
        assert np.all(counts.reshape(-1, 3)[~np.isfinite(F).all(axis=2)] == 0)
    engine.set_fundamental_metric(0)


def test_six_correspondences_are_refused(mh, engine):
    src, dst = _scene(7)
    engine.set_correspondences(src[:6], dst[:6])
    with pytest.raises(mh.MultiHError) as ei:
        engine.propose_fund7(1, 0, 4)
    assert ei.value.code == MH_ERR_INVALID


# ---- scoring reuse -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_scores_over_the_slots(engine, metric):
    n, m = 64, 65
    src, dst = _scene(n)
    engine.set_correspondences(src, dst)
    engine.set_fundamental_metric(metric)
    try:
        F, idx, nvalid = _propose(engine, 31, 0, m)
        thr2 = 2.0 * 2.0
        counts = engine.score_sampson(thr2).reshape(m, 3)
    finally:
        engine.set_fundamental_metric(0)
    lo = np.zeros((m, 3), dtype=np.int64)
    hi = np.zeros((m, 3), dtype=np.int64)
    for s in range(m):
        for j in range(3):
            lo[s, j], hi[s, j] = T.count_bounds(F[s, j], src, dst, thr2, metric)
    assert np.all((lo <= counts) & (counts <= hi)), "a count differs from the documented formula beyond the points at thr^2"
    assert np.all(counts[~np.isfinite(F).all(axis=2)] == 0)
    assert counts.max() >= 7


# ---- stop rule and estimator -----------------------------------------------------------------------------------------------------
def test_exact_inliers_stop_after_one_sample(engine):
    n = 64
    src, dst = _scene(n, noise=0.0)
    engine.set_correspondences(src, dst)
    F, e2, mask, inl, used = engine.estimate_fundamental_minimal(7, 200, 0.99, 1.0)
    assert used == 1 and inl == n and mask.sum() == n
    assert np.all(np.isfinite(F)) and np.all(np.isfinite(e2))


def _mixed(inliers, outliers, seed):
    src, dst = _scene(inliers + outliers)
    us, ud = T.uniform_rows(outliers, seed)
    return (np.ascontiguousarray(np.concatenate([src[:inliers], us])),
            np.ascontiguousarray(np.concatenate([dst[:inliers], ud])))


@pytest.mark.parametrize("inliers,outliers", [(32, 32), (56, 8)])
@pytest.mark.parametrize("metric", [0, 1])
def test_estimator_follows_the_replay(engine, inliers, outliers, metric):
    """32 + 32: the case of the definition (N stays above 200, every sample is used).  56 + 8 is there for the stop itself:
    w = 7/8 gives N = 10, so the run ends in the middle of the batch and later, better samples must not be seen."""
    n, S, c, thr = inliers + outliers, 200, 0.99, 2.0
    src, dst = _mixed(inliers, outliers, seed=3)
    engine.set_correspondences(src, dst)
    engine.set_fundamental_metric(metric)
    try:
        for seed in range(40, 48):       # a seed whose replay passes within 1e-9 of an integer quotient is replaced
            engine.propose_fund7(seed, 0, S)
            counts = engine.score_sampson(thr * thr)
            used, win, best, margin = T.ransac_stop_replay(counts, n, c)
            if margin > 1e-9:
                break
        else:
            pytest.fail("no seed with a decidable replay")
        Fh = engine.get_fund7_hypotheses().reshape(-1, 9)
        F, e2, mask, inl, used_gpu = engine.estimate_fundamental_minimal(seed, S, c, thr)
    finally:
        engine.set_fundamental_metric(0)
    print(f"{inliers}+{outliers}, metric {metric}, seed {seed}: samples_used {used_gpu} (replay {used}), slot {win}, count {best}")
    assert used_gpu == used
    assert np.array_equal(F.view(np.uint64), Fh[win].view(np.uint64)), "the returned F is not the winning slot's"
    assert inl == int(mask.sum()) == best == int(counts[win])
    assert win == int(np.argmax(counts[:3 * used]))                  # ties go to the lowest index
    assert np.all(np.isfinite(e2))
    if (inliers, outliers) == (56, 8):
        assert used < S


def test_small_inlier_ratio_never_stops_early(engine):
    """4 000 uniform rows and 12 exact inliers at 0.05 px: a sample explains little more than its own seven points, so
    w = best / n stays below 0.004, where 1 - w^7 rounds to 1 in float64 and a plain log(1 - w^7) is 0.  N(s) is in truth
    ~ 4.6 / w^7 > 1e17 and clamps to S: every sample is used.  (A quotient that came out as -inf would end the run after
    one sample.)"""
    n, S, c, thr = 4012, 200, 0.99, 0.05
    src_i, dst_i = _scene(64, noise=0.0)
    us, ud = T.uniform_rows(4000, seed=21)
    src = np.ascontiguousarray(np.concatenate([src_i[:12], us]))
    dst = np.ascontiguousarray(np.concatenate([dst_i[:12], ud]))
    engine.set_correspondences(src, dst)
    for metric in (0, 1):
        engine.set_fundamental_metric(metric)
        try:
            engine.propose_fund7(61, 0, S)
            counts = engine.score_sampson(thr * thr)
            Fh = engine.get_fund7_hypotheses().reshape(-1, 9)
            F, e2, mask, inl, used_gpu = engine.estimate_fundamental_minimal(61, S, c, thr)
        finally:
            engine.set_fundamental_metric(0)
        used, win, best, margin = T.ransac_stop_replay(counts, n, c)
        print(f"metric {metric}: best count {best} of {n} (w = {best / n:.2g}), samples_used {used_gpu} (replay {used})")
        assert 7 <= counts[:3].max() and counts.max() / n < 0.004, "the case must pass through w < 0.004 from its first sample on"
        assert 1.0 - (counts.max() / n) ** 7 == 1.0
        assert used == S and used_gpu == S
        assert np.array_equal(F.view(np.uint64), Fh[win].view(np.uint64)) and inl == int(mask.sum()) == best


def test_uniform_rows_use_every_sample_or_fail(mh, engine):
    n, S = 64, 50
    src, dst = T.uniform_rows(n, seed=9)
    engine.set_correspondences(src, dst)
    try:
        F, e2, mask, inl, used = engine.estimate_fundamental_minimal(13, S, 0.99, 0.01)
    except mh.MultiHError as err:
        assert err.code == MH_ERR_INVALID
        engine.propose_fund7(13, 0, S)
        assert engine.score_sampson(1e-4).max() == 0
    else:
        assert used == S and np.all(np.isfinite(F)) and 1 <= inl == int(mask.sum()) < n


def test_argument_checks(mh, engine):
    src, dst = _scene(64)
    engine.set_correspondences(src, dst)
    F, e2, mask, inl, used = engine.estimate_fundamental_minimal(3, 1, 0.99, 2.0)
    assert used == 1 and np.all(np.isfinite(F)) and inl == int(mask.sum()) >= 7
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(mh.MultiHError) as ei:
            engine.estimate_fundamental_minimal(3, 10, bad, 2.0)
        assert ei.value.code == MH_ERR_INVALID
    with pytest.raises(mh.MultiHError) as ei:
        engine.estimate_fundamental_minimal(3, 0, 0.99, 2.0)
    assert ei.value.code == MH_ERR_INVALID


# ---- host route ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_host_route(mh, engine, metric):
    n, thr, seed = 64, 2.0, 77
    src, dst = _mixed(48, 16, seed=4)
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_fundamental_estimator.argtypes = [C.c_int, C.c_int, C.c_double]
    host.mhh_set_fundamental_estimator.restype = None
    dp = C.POINTER(C.c_double)

    def filtered():
        mask = np.zeros(n, dtype=np.uint8)
        kept = host.mhh_filter_correspondences(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), n, C.c_double(thr),
                                               C.c_ulonglong(seed), 500, metric, 0, mask.ctypes.data_as(C.POINTER(C.c_ubyte)))
        assert kept == int(mask.sum())
        return mask

    engine.set_correspondences(src, dst)
    engine.set_fundamental_metric(metric)
    try:
        host.mhh_set_fundamental_estimator(1, 200, 0.99)
        minimal = filtered()
        host.mhh_set_fundamental_estimator(-1, 0, 0.0)
        default = filtered()
        want_minimal = engine.estimate_fundamental_minimal(seed, 200, 0.99, thr)[2]
        want_default = engine.estimate_fundamental(seed, 500, thr)[2]
    finally:
        host.mhh_set_fundamental_estimator(-1, 0, 0.0)
        engine.set_fundamental_metric(0)
    assert np.array_equal(minimal, want_minimal)
    assert np.array_equal(default, want_default)


def test_process_honours_the_hook(mh, engine, synth):
    """mhh_run_process without a given F: with mhh_set_fundamental_estimator(1, 200, 0.99) the rows in Process()'s RANSAC
    mask are those of mh_estimate_fundamental_minimal with Process()'s seed (proposal seed ^ 0xf00d) and threshold, after
    mhh_set_fundamental_estimator(-1, ...) those of mh_estimate_fundamental; an unknown mode makes Process() and the filter fail."""
    seed, thr_f = 5, 2.6
    sc = synth.make_scene(1500, 3, seed=31, outlier_frac=0.3, with_neighbours=False)
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_fundamental_estimator.argtypes = [C.c_int, C.c_int, C.c_double]
    host.mhh_set_fundamental_estimator.restype = None
    dp = C.POINTER(C.c_double)
    src, dst, aff = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff))

    def process():
        labels = np.full(sc.n, -7, dtype=np.int32)
        Hout = np.zeros((64, 9))
        it, en = C.c_int(-1), C.c_double(-1)
        k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, None, None,
                                 C.c_double(thr_f), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(seed),
                                 2000, 8, 0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)), Hout.ctypes.data_as(dp), 64,
                                 C.byref(it), C.byref(en), None, 0, 4)
        st = (C.c_int * 4)()
        host.mhh_get_front_stages(st)
        return k, list(st)

    engine.set_fundamental_metric(1)                    # the class default
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    try:
        host.mhh_set_fundamental_estimator(1, 200, 0.99)
        k_min, st_min = process()
        host.mhh_set_fundamental_estimator(2, 200, 0.99)
        k_bad, _ = process()
        mask = np.zeros(sc.n, dtype=np.uint8)
        kept_bad = host.mhh_filter_correspondences(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), sc.n, C.c_double(2.0), C.c_ulonglong(seed),
                                                   500, 1, 0, mask.ctypes.data_as(C.POINTER(C.c_ubyte)))
        host.mhh_set_fundamental_estimator(-1, 0, 0.0)
        k_def, st_def = process()
        inl_min = engine.estimate_fundamental_minimal(seed ^ 0xf00d, 200, 0.99, thr_f)[3]
        inl_def = engine.estimate_fundamental(seed ^ 0xf00d, 4000, thr_f)[3]
    finally:
        host.mhh_set_fundamental_estimator(-1, 0, 0.0)
        engine.set_fundamental_metric(0)
    assert k_min >= 1 and st_min[0] == sc.n and st_min[1] == inl_min
    assert k_def >= 1 and st_def[1] == inl_def
    assert k_bad == -1 and kept_bad == -1


# ---- the default route is untouched ----------------------------------------------------------------------------------------------
def test_eight_point_route_after_a_seven_point_proposal(mh, engine):
    src, dst = _scene(64)
    with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as fresh:
        fresh.set_correspondences(src, dst)
        fresh.propose_fund8(17, 2, 40)
        F_want, idx_want = fresh.get_fund_hypotheses()
    engine.set_correspondences(src, dst)
    engine.propose_fund7(17, 0, 70)
    with pytest.raises(mh.MultiHError) as ei:          # seven indices per sample: not readable as m x 8
        engine.get_fund_hypotheses()
    assert ei.value.code == MH_ERR_INVALID
    engine.propose_fund8(17, 2, 40)
    F, idx = engine.get_fund_hypotheses()
    assert np.array_equal(F.view(np.uint64), F_want.view(np.uint64)) and np.array_equal(idx, idx_want)
