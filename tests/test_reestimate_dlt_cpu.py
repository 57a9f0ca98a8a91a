"""CPU tests of the yardsticks of the per-label N-point DLT estimator and of the epipolar-free route: the per-label wrapper
(tests/reestimate_dlt_numpy.py::reestimate over refit_h_numpy.fit, the kernel's twin) against the plain definition of the fit
(refit_h_numpy.fit_plain: the 2 c x 9 design matrix and numpy.linalg.svd), its keep-on-failure cases, the three-motion scene's
separation, and the host's medoid merge candidates (mhh_merge_candidates_medoid) against the numpy rule."""
import ctypes as C
import os

import numpy as np
import pytest

import reestimate_dlt_numpy as D
import refit_h_numpy as R

_dp = C.POINTER(C.c_double)
SIZES = (4, 5, 6, 7, 9, 40, 64, 257, 300, 513)
TOL = 1e-6                         # the project's tolerance for homographies (unit norm, sign fixed)


@pytest.fixture(scope="module")
def host(mh, engine_lib):
    return C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))


def _labelled_sets(sizes, seed, outliers=60, noise=0.5):
    """Label sets of the given sizes, each on a plane of its own, scattered through arrays with outlier rows (label -1)."""
    rng = np.random.default_rng(seed)
    n = sum(sizes) + outliers
    src = rng.uniform(0, 1000, size=(n, 2))
    dst = rng.uniform(0, 1000, size=(n, 2))
    labels = np.full(n, -1, dtype=np.int32)
    perm = rng.permutation(n)
    at = 0
    for k, c in enumerate(sizes):
        idx = np.sort(perm[at:at + c])
        at += c
        s, d, _, _ = R.plane_scene(rng, c, noise)
        src[idx], dst[idx] = s, d
        labels[idx] = k
    return src, dst, labels


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_wrapper_equals_the_plain_definition(seed):
    src, dst, labels = _labelled_sets(SIZES, seed)
    H_in = np.tile(np.eye(3).reshape(9), (len(SIZES), 1))
    H, counts = D.reestimate(src, dst, labels, H_in)
    assert counts.tolist() == list(SIZES)
    for k, c in enumerate(SIZES):                          # no set is left out
        idx = np.flatnonzero(labels == k)
        plain = R.fit_plain(src, dst, idx)
        err = np.abs(R.unit_sign(H[k]) - plain).max()
        print(f"seed {seed} members {c}: |twin - svd| = {err:.3e}")
        assert err <= TOL, (seed, c, err)
        assert R.same_bits(H[k], R.fit(src, dst, idx))


def test_labels_outside_the_model_set_belong_to_nobody():
    src, dst, labels = _labelled_sets((40, 9), 5)
    extra = labels.copy()
    free = np.flatnonzero(labels == -1)
    extra[free[:10]] = 2                                   # >= Nh
    extra[free[10:20]] = 77
    H_in = np.tile(np.eye(3).reshape(9), (2, 1))
    a, ca = D.reestimate(src, dst, labels, H_in)
    b, cb = D.reestimate(src, dst, extra, H_in)
    assert R.same_bits(a, b) and np.array_equal(ca, cb)


def _failure_cases():
    rng = np.random.default_rng(9)
    src, dst, labels = _labelled_sets((3, 40, 16, 30), 9)
    # label 0: 3 members; label 1: a healthy set; label 2: all members the same point; label 3: a NaN coordinate in a member;
    # label 4: no members.  (The same point 16 times, integer coordinates: the sums and the scale by 1 / 16 are exact, so the
    # centroid is the point itself, both mean distances are 0 and the scales are not finite.  Where the centroid rounds away
    # from the point the scales are finite and the fit is defined.)
    same = np.flatnonzero(labels == 2)
    src[same], dst[same] = np.floor(src[same[0]]), np.floor(dst[same[0]])
    dst[np.flatnonzero(labels == 3)[4], 1] = np.nan
    H_in = rng.normal(size=(5, 9))
    return src, dst, labels, H_in


def test_failed_fits_keep_their_models():
    src, dst, labels, H_in = _failure_cases()
    H, counts = D.reestimate(src, dst, labels, H_in)
    assert counts.tolist() == [3, 40, 16, 30, 0]
    for k in (0, 2, 3, 4):
        assert R.same_bits(H[k], H_in[k]), k
    assert not R.same_bits(H[1], H_in[1])
    assert np.abs(R.unit_sign(H[1]) - R.fit_plain(src, dst, np.flatnonzero(labels == 1))).max() <= TOL


def test_three_motion_scene_is_separated_and_deterministic():
    a, b = D.three_motions(1200), D.three_motions(1200)
    assert np.array_equal(a.src, b.src) and np.array_equal(a.dst, b.dst) and np.array_equal(a.hit_col, b.hit_col)
    assert D.separated([h.reshape(3, 3) for h in a.H_true])
    assert sorted(np.unique(a.gt_label).tolist()) == [-1, 0, 1, 2]
    assert 0.2 < (a.gt_label < 0).mean() < 0.3
    assert np.diff(a.hit_rowptr).min() >= 16
    for k in range(3):                                     # every strip's inliers fit its own H, and nobody else's
        m = a.gt_label == k
        assert m.sum() > 200
        d = np.sqrt(R.d2_of(a.src[m], a.dst[m], a.H_true[k]))
        assert np.median(d) < 1.0
        for j in range(3):
            if j != k:
                assert np.sqrt(R.d2_of(a.src[m], a.dst[m], a.H_true[j])).min() > 8.0


# ---- the medoid merge candidates ----------------------------------------------------------------------------------------------

def _medoid_hook(host, H, thr_h, seed):
    H = np.ascontiguousarray(H, dtype=np.float64).reshape(-1, 9)
    nh = H.shape[0]
    feat, modes, cand = np.zeros((nh, 6)), np.zeros((nh, 6)), np.zeros((nh, 9))
    cand_mode = np.zeros(nh, np.int32)
    k, draws = C.c_int(0), C.c_ulonglong(0)
    nc = host.mhh_merge_candidates_medoid(H.ctypes.data_as(_dp), nh, C.c_double(thr_h), C.c_ulonglong(seed), feat.ctypes.data_as(_dp),
                                          modes.ctypes.data_as(_dp), C.byref(k), cand.ctypes.data_as(_dp),
                                          cand_mode.ctypes.data_as(C.POINTER(C.c_int)), C.byref(draws))
    return feat, modes[:k.value].copy(), cand[:nc].copy(), cand_mode[:nc].copy(), int(draws.value)


def _members(host, feat, thr_h, seed):
    """The members of every mode, from the host's own mean shift with the same draws."""
    nh = feat.shape[0]
    assign = np.zeros(nh, np.int32)
    modes = np.zeros((nh, 6))
    k = host.mhh_mean_shift(np.ascontiguousarray(feat).ctypes.data_as(_dp), nh, 6, C.c_double(thr_h), C.c_ulonglong(seed),
                            modes.ctypes.data_as(_dp), nh, assign.ctypes.data_as(C.POINTER(C.c_int)), None)
    return [np.flatnonzero(assign == c) for c in range(k)]


def _far_apart(rng, m):
    H = np.tile(np.eye(3).reshape(9), (m, 1)) + rng.normal(0, 0.02, size=(m, 9))
    H[:, 2] = 100.0 * np.arange(m) + rng.uniform(-5, 5, m)           # features at least 90 apart
    H[:, 8] = 1.0
    return np.ascontiguousarray(H)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_medoid_candidates_equal_the_numpy_rule(host, seed):
    rng = np.random.default_rng(seed)
    base = _far_apart(rng, 5)
    H = np.concatenate([base[k] * (1 + rng.normal(0, 2e-5, size=(int(rng.integers(1, 6)), 9))) for k in range(5)])
    H = np.ascontiguousarray(H[rng.permutation(len(H))])
    feat, modes, cand, cand_mode, draws = _medoid_hook(host, H, 2.2, 7 * seed + 1)
    assert R.same_bits(feat, D.features(H))
    members = _members(host, feat, 2.2, 7 * seed + 1)
    assert len(members) == len(modes) == 5
    want, want_mode = D.medoid_candidates(H, feat, modes, members)
    assert R.same_bits(cand, want) and np.array_equal(cand_mode, want_mode)
    for c in cand:                                         # every candidate is one of the inputs, nine doubles unchanged
        assert any(R.same_bits(c, h) for h in H)


def test_models_far_apart_come_back_unchanged(host):
    H = _far_apart(np.random.default_rng(11), 7)
    feat, modes, cand, cand_mode, _ = _medoid_hook(host, H, 2.2, 5)
    assert len(modes) == 7 and cand_mode.tolist() == list(range(7))
    members = _members(host, feat, 2.2, 5)
    order = [int(m[0]) for m in members]                   # one member per mode: the candidates are the inputs, in mode order
    assert sorted(order) == list(range(7))
    assert R.same_bits(cand, H[order])


def test_two_models_inside_one_band_width_give_one_of_them(host):
    rng = np.random.default_rng(12)
    H = _far_apart(rng, 3)
    H = np.ascontiguousarray(np.concatenate([H, H[1:2]]))
    H[3, 2] += 0.7                                         # 0.7 away from model 1 in three of the six features: 2.1 in L1
    feat, modes, cand, cand_mode, _ = _medoid_hook(host, H, 2.2, 3)
    assert len(modes) == 3 and len(cand) == 3
    pair = [c for c in cand if R.same_bits(c, H[1]) or R.same_bits(c, H[3])]
    assert len(pair) == 1
    assert sum(R.same_bits(c, H[0]) for c in cand) == 1 and sum(R.same_bits(c, H[2]) for c in cand) == 1


def test_a_tie_takes_the_lower_index(host):
    rng = np.random.default_rng(13)
    H = _far_apart(rng, 3)
    H = np.ascontiguousarray(np.concatenate([H[:2], H[1:2], H[2:]]))      # models 1 and 2 are the same nine doubles
    feat, modes, cand, cand_mode, _ = _medoid_hook(host, H, 2.2, 4)
    members = _members(host, feat, 2.2, 4)
    twin_mode = [c for c, m in enumerate(members) if 1 in m.tolist()]
    assert len(twin_mode) == 1 and sorted(members[twin_mode[0]].tolist()) == [1, 2]
    want, _ = D.medoid_candidates(H, feat, modes, members)
    assert R.same_bits(cand, want)
    # the rule itself, where the bits cannot tell: equal distances give the lower index
    f = np.array([[0.0] * 6, [1.0] + [0.0] * 5, [-1.0] + [0.0] * 5])
    Hs = np.arange(27, dtype=np.float64).reshape(3, 9)
    got, _ = D.medoid_candidates(Hs, f, np.zeros((1, 6)), [np.array([2, 1])])
    assert R.same_bits(got[0], Hs[1])


def test_a_distance_that_is_not_a_number_loses(host):
    """The rule: a member whose feature distance is NaN never wins against one whose distance is a number, wherever it stands;
    members that are all NaN give the lowest index.  (The host's mean shift never makes a row with a NaN feature a member of a
    mode with other members — its L1 ball test is false for it — so the hook cannot be driven there: the rule is held here, and
    the hook on a model set with such a row still equals it.)"""
    Hs = np.arange(36, dtype=np.float64).reshape(4, 9)
    nan = [np.nan] + [0.0] * 5
    f = np.array([nan, [2.0] + [0.0] * 5, nan, [1.0] + [0.0] * 5])
    pick = lambda mem: D.medoid_candidates(Hs, f, np.zeros((1, 6)), [np.array(mem)])[0][0]
    assert R.same_bits(pick([0, 1, 2, 3]), Hs[3])
    assert R.same_bits(pick([0, 1]), Hs[1]) and R.same_bits(pick([1, 2]), Hs[1])
    assert R.same_bits(pick([2, 0]), Hs[0])
    H = _far_apart(np.random.default_rng(14), 4)
    H[2, 8] = 0.0                                          # h33 = 0: two of its six features are infinite, none is finite in L1
    feat, modes, cand, cand_mode, _ = _medoid_hook(host, H, 2.2, 6)
    members = _members(host, feat, 2.2, 6)
    want, want_mode = D.medoid_candidates(H, feat, modes, members)
    assert R.same_bits(cand, want) and np.array_equal(cand_mode, want_mode)
    assert all(any(R.same_bits(c, h) for h in H) for c in cand)
