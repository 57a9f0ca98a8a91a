"""mh_refit_homography (csrc/refit_h.hip, k_refit_h) and the refitting degenerate tail (MultiH::SetTailRefit) on the GPU,
against the numpy twin of the rule in include/multih_hip.h (tests/refit_h_numpy.py): H_out as uint64 bits, the inlier flags,
the count and the number of accepted fits exactly.  The seeds of the round cases were found on the CPU with the twin; every
such case asserts that it is what it was chosen for."""
import ctypes as C
import os

import numpy as np
import pytest

import refit_h_numpy as T
import test_gpu_alternation as alt

pytestmark = pytest.mark.gpu
THR2 = 2.2 * 2.2
IDENT = np.eye(3).reshape(9)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _held_to_the_twin(engine, src, dst, H_in, thr2, iterations):
    """One call against the twin; returns the twin's (H, mask, inliers, accepted, why)."""
    why = []
    H, mask, inl, acc = T.refit(src, dst, H_in, thr2, iterations, why)
    gH, gmask, ginl, gacc = engine.refit_homography(H_in, thr2, iterations)
    assert (ginl, gacc) == (inl, acc), (iterations, (ginl, gacc), (inl, acc), why)
    assert np.array_equal(gmask, mask), int((gmask != mask).sum())
    assert np.array_equal(_bits(gH), _bits(H)), (gH, H)
    return H, mask, inl, acc, why[0]


def _start_from_four(src, dst, good, rng):
    return T.fit(src, dst, np.sort(rng.choice(np.flatnonzero(good), 4, replace=False)))


@pytest.mark.parametrize("n", [4, 5, 255, 256, 257, 513, 2000])
def test_stride_and_membership_edges(engine, n):
    """The sizes at which the 256-thread sums change shape: fewer points than threads, exactly one per thread, one thread with
    two, two full trips and one over, many trips; 30 % outliers, so the members of a thread are not consecutive trips."""
    rng = np.random.default_rng(n)
    outliers = int(0.3 * n)
    src, dst, H_true, good = T.plane_scene(rng, n - outliers, 0.7, outliers=outliers)
    # the start: a fit to eight of the plane's points (a 4-point fit at this noise may explain its own four points alone)
    H_in = T.fit(src, dst, np.sort(rng.choice(np.flatnonzero(good), 8, replace=False))) if good.sum() > 8 else H_true
    engine.set_correspondences(src, dst)
    seen = [_held_to_the_twin(engine, src, dst, H_in, THR2, it) for it in (0, 1, 3)]
    if n >= 255:
        assert seen[2][3] >= 1 and seen[2][2] > 0.5 * good.sum()            # (not vacuous: a fit was made and kept)


def test_inlier_sets_of_exactly_four_and_three(engine):
    rng = np.random.default_rng(17)
    src, dst, H_true, good = T.plane_scene(rng, 4, 0.0, outliers=300)
    engine.set_correspondences(src, dst)
    assert T.refit(src, dst, H_true, 1e-6, 0)[2] == 4
    H, mask, inl, acc, why = _held_to_the_twin(engine, src, dst, H_true, 1e-6, 2)
    assert inl == 4 and np.array_equal(mask.astype(bool), good)
    # one of the four moved away: three inliers, no fit, H_in comes back
    dst3 = dst.copy()
    dst3[np.flatnonzero(good)[2]] += 50.0
    engine.set_correspondences(src, dst3)
    H, mask, inl, acc, why = _held_to_the_twin(engine, src, dst3, H_true, 1e-6, 2)
    assert (inl, acc, why) == (3, 0, "fit failed") and np.array_equal(_bits(H), _bits(H_true))


def test_threshold_on_a_residual_value_and_nan_model(engine):
    rng = np.random.default_rng(23)
    src, dst, H_true, good = T.plane_scene(rng, 600, 1.0, outliers=250)
    engine.set_correspondences(src, dst)
    H_in = _start_from_four(src, dst, good, rng)
    d2 = T.d2_of(src, dst, H_in)
    k = int(np.argsort(d2)[300])                                             # a point in the middle of the inliers
    thr2 = float(d2[k])
    for it in (0, 2):
        _held_to_the_twin(engine, src, dst, H_in, thr2, it)
    _, mask, inl, _ = engine.refit_homography(H_in, thr2, 0)
    assert mask[k] == 0 and inl == 300                                       # strictly below: the point ON the threshold is out
    _, mask, inl, _ = engine.refit_homography(H_in, float(np.nextafter(thr2, np.inf)), 0)
    assert mask[k] == 1 and inl == 301
    # a NaN model has no inliers and comes back as it came
    H_nan = H_in.copy()
    H_nan[4] = np.nan
    H, mask, inl, acc, why = _held_to_the_twin(engine, src, dst, H_nan, THR2, 3)
    assert (inl, acc, why) == (0, 0, "fit failed") and not mask.any() and np.array_equal(_bits(H), _bits(H_nan))


def _one_plane_1500(seed):
    rng = np.random.default_rng(seed)
    src, dst, _, good = T.plane_scene(rng, 1050, 1.0, outliers=450)
    return src, dst, T.fit(src, dst, rng.choice(np.flatnonzero(good), 4, replace=False))


def test_rounds_from_a_four_point_hypothesis(engine):
    """iterations 0 .. 4 on 1 500 points of one plane: the counts never fall and several fits are accepted; with room for
    it the rounds end on their own, at a fixed point (the candidate has the bits of what stands)."""
    src, dst, H0 = _one_plane_1500(1)
    engine.set_correspondences(src, dst)
    seen = [_held_to_the_twin(engine, src, dst, H0, THR2, it) for it in range(5)]
    counts = [s[2] for s in seen]
    assert np.array_equal(_bits(seen[0][0]), _bits(H0)) and seen[0][3] == 0
    assert all(b >= a for a, b in zip(counts, counts[1:])) and counts[4] > 3 * counts[0]
    assert seen[4][3] >= 2 and [s[3] for s in seen] == [0, 1, 2, 3, 4]
    H, mask, inl, acc, why = _held_to_the_twin(engine, src, dst, H0, THR2, 16)
    assert why == "same bits" and 4 < acc < 16 and inl >= counts[4]


def _two_planes(seed):
    rng = np.random.default_rng(100 + seed)
    s1, d1, H1, _ = T.plane_scene(rng, 500, 0.5)
    s2, d2, H2, _ = T.plane_scene(rng, 500, 0.5, outliers=200)
    src, dst = np.concatenate([s1, s2]), np.concatenate([d1, d2])
    perm = rng.permutation(src.shape[0])
    return np.ascontiguousarray(src[perm]), np.ascontiguousarray(dst[perm]), T.unit_sign(0.5 * (H1 + H2))


@pytest.mark.parametrize("seed,thr,accepted_before", [(4, 120.0, 0), (1, 60.0, 2)])
def test_a_refit_that_explains_fewer_points_is_dropped(engine, seed, thr, accepted_before):
    """A model between two planes under a wide threshold collects points of both; the least-squares fit to that mixture
    explains fewer of them.  The refit is dropped and the flags are those of the model that stands."""
    src, dst, H_mid = _two_planes(seed)
    engine.set_correspondences(src, dst)
    H, mask, inl, acc, why = _held_to_the_twin(engine, src, dst, H_mid, thr * thr, 4)
    assert why == "fewer inliers" and acc == accepted_before
    if acc == 0:
        assert np.array_equal(_bits(H), _bits(H_mid))
    assert np.array_equal(mask.astype(bool), T.inlier_mask(src, dst, H, thr * thr)) and inl == int(mask.sum())


def test_fits_that_fail_or_degenerate(engine):
    rng = np.random.default_rng(31)
    # all inliers coincident: 32 copies of (512, 128) -> (256, 64) under H = diag(.5, .5, 1), everything else far from it.
    # The sums of the copies and 1.0 / 32 are exact, the centroid is the point, the mean distance 0, the scale infinite.
    n = 700
    src = rng.uniform(0, 1000, size=(n, 2))
    dst = 0.5 * src + 300.0
    at = rng.choice(n, 32, replace=False)
    src[at], dst[at] = [512.0, 128.0], [256.0, 64.0]
    H_in = np.diag([0.5, 0.5, 1.0]).reshape(9)
    engine.set_correspondences(src, dst)
    H, mask, inl, acc, why = _held_to_the_twin(engine, src, dst, H_in, THR2, 3)
    assert (inl, acc, why) == (32, 0, "fit failed") and np.array_equal(_bits(H), _bits(H_in))
    assert np.array_equal(np.flatnonzero(mask), np.sort(at))
    # collinear inliers: the normal matrix has a null space of more than one dimension; whatever the rule gives
    src, dst, H_true, good = T.plane_scene(rng, 40, 0.0, outliers=400)
    g = np.flatnonzero(good)
    src[g] = np.stack([25.0 * np.arange(40), 3.0 + 0.5 * 25.0 * np.arange(40)], axis=1)
    q = np.concatenate([src[g], np.ones((40, 1))], axis=1) @ H_true.reshape(3, 3).T
    dst[g] = q[:, :2] / q[:, 2:3]
    engine.set_correspondences(src, dst)
    assert T.refit(src, dst, H_true, 1e-6, 0)[2] == 40
    for it in (1, 3):
        _held_to_the_twin(engine, src, dst, H_true, 1e-6, it)


def test_engine_state_is_untouched(engine):
    src, dst, H0 = _one_plane_1500(2)
    engine.set_correspondences(src, dst)

    def run(with_refit):
        engine.propose_dlt4(77, 0, 600)
        counts = engine.score(THR2)
        if with_refit:
            engine.refit_homography(H0, THR2, 3)
        best = engine.select_best()
        if with_refit:
            engine.refit_homography(H0, THR2, 1)
        return engine.model_count, engine.get_models(), counts, best, engine.score(THR2)

    plain, mixed = run(False), run(True)
    assert plain[0] == mixed[0] == 600 and plain[3] == mixed[3] and plain[3][1] == int(plain[2].max())
    assert np.array_equal(_bits(plain[1]), _bits(mixed[1]))
    assert np.array_equal(plain[2], mixed[2]) and np.array_equal(plain[4], mixed[4]) and np.array_equal(plain[2], plain[4])


def test_error_codes(mh, engine):
    lib, h = engine.lib, engine._h
    dp = C.POINTER(C.c_double)
    H, out = IDENT.copy(), np.empty(9)
    Hp, op = H.ctypes.data_as(dp), out.ctypes.data_as(dp)
    call = lambda *a: lib.mh_refit_homography(*a, None, None, None)
    assert call(h, Hp, C.c_double(1.0), 1, op) == -4                         # MH_ERR_NOT_SET: no correspondences yet
    src, dst, _ = _one_plane_1500(3)
    engine.set_correspondences(src[:50], dst[:50])
    assert call(h, Hp, C.c_double(1.0), 1, op) == 0
    assert call(None, Hp, C.c_double(1.0), 1, op) == -2
    assert call(h, None, C.c_double(1.0), 1, op) == -2
    assert call(h, Hp, C.c_double(1.0), 1, None) == -2
    assert call(h, Hp, C.c_double(1.0), -1, op) == -2
    assert call(h, Hp, C.c_double(1.0), 17, op) == -2
    assert call(h, Hp, C.c_double(float("nan")), 1, op) == -2
    assert call(h, Hp, C.c_double(1.0), 0, op) == 0 and call(h, Hp, C.c_double(np.inf), 16, op) == 0
    with pytest.raises(mh.capi.MultiHError):
        engine.refit_homography(IDENT, 1.0, 17)


@pytest.mark.parametrize("tail_score", [0, 1])
def test_the_degenerate_tail_refits_its_winner(mh, engine_lib, synth, oracle, tail_score):
    """The one-plane scene of test_gpu_alternation.test_process_ends_in_the_degenerate_tail_like_the_oracle.  With
    SetTailRefit(3) Process() returns the twin's refit of what the default tail returns — the winner by count or by MSAC
    weight — and labels that refit's inliers on the original points; with 0 it is the default run bit for bit."""
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    for fn in (host.mhh_set_tail_refit, host.mhh_set_tail_score):
        fn.argtypes, fn.restype = [C.c_int], None
    sc = synth.make_scene(1500, 1, seed=41, with_neighbours=False)
    H0 = alt._initial_models(sc, 41, 1, 1)
    try:
        host.mhh_set_tail_score(tail_score)
        k0, labels0, Hd, it0, en0 = alt._run_process(mh, sc, 41, H0=H0)
        host.mhh_set_tail_refit(3)
        k3, labels3, H3, _, _ = alt._run_process(mh, sc, 41, H0=H0)
        host.mhh_set_tail_refit(0)
        kz, labelsz, Hz, itz, enz = alt._run_process(mh, sc, 41, H0=H0)
        host.mhh_set_tail_refit(17)
        k17 = alt._run_process(mh, sc, 41, H0=H0)[0]
    finally:
        host.mhh_set_tail_refit(-1)
        host.mhh_set_tail_score(-1)
    assert k0 == k3 == kz == 1 and k17 == -1
    assert np.array_equal(labels0 == 0, T.inlier_mask(sc.src, sc.dst, Hd[0], alt.THR * alt.THR))      # (the default tail, as ever)
    H, mask, inl, acc = T.refit(sc.src, sc.dst, Hd[0], alt.THR * alt.THR, 3)
    assert acc >= 1, "the scene should let the refit change the model"
    assert np.array_equal(_bits(H3[0]), _bits(H))
    assert np.array_equal(labels3, np.where(mask, 0, -1))
    assert (labels3 == 0).sum() >= (labels0 == 0).sum()
    assert np.array_equal(labelsz, labels0) and np.array_equal(_bits(Hz), _bits(Hd)) and (itz, enz) == (it0, en0)
