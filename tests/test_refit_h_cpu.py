"""CPU tests of the homography refit (mh_refit_homography): the numpy twin (tests/refit_h_numpy.py) against the plain
definition of the same fit (design matrix + SVD), the failures of fit(S), the round rule on hand-made sequences, and what the
libraries must export.  Nothing here needs a GPU; tests/test_gpu_refit_h.py holds the kernel to the twin."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import refit_h_numpy as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4, 5, 8, 50, 300, 2000)
NOISES = (0.0, 0.5, 1.5)
SEEDS = (1, 2, 3, 4)
TOL = 1e-6                       # the project's homography tolerance
WITNESS = 1e-6                   # second-smallest eigenvalue of the normal matrix below this share of the largest: left out
MAX_LEFT_OUT = 0.05


def test_strided_tree_sum_is_the_engines_order(oracle):
    """The vectorised sum against the order written out: thread t adds its members one by one, then the tree."""
    rng = np.random.default_rng(7)
    for n, keep in ((1, 1.0), (255, 0.5), (256, 1.0), (257, 1.0), (1300, 0.3), (1300, 1.0)):
        idx = np.flatnonzero(rng.random(n) < keep)
        terms = rng.normal(0, 1e3, size=(idx.size, 3)) * 10.0 ** rng.integers(-8, 8, size=(idx.size, 1))
        acc = [[0.0] * 3 for _ in range(T.LANES)]
        for j, i in enumerate(idx):
            for k in range(3):
                acc[i % T.LANES][k] = acc[i % T.LANES][k] + float(terms[j, k])
        s = 128
        while s >= 1:
            for t in range(s):
                for k in range(3):
                    acc[t][k] = acc[t][k] + acc[t + s][k]
            s //= 2
        assert T.same_bits(T.strided_tree_sum(idx, terms), np.array(acc[0]))


def test_twin_fit_is_the_plain_definition(oracle):
    """fit(S) through the 24 strided sums, the 9 x 9 normal matrix and the cyclic Jacobi against the 2 c x 9 design matrix
    and numpy's SVD on the same normalised points, after unit norm and sign.  A normal-equation fit squares the condition
    number: a case is left out only when its own eigenvalues say the null vector is not determined to TOL."""
    cases = left_out = 0
    worst = 0.0
    for c in SIZES:
        for noise in NOISES:
            for seed in SEEDS:
                rng = np.random.default_rng(1000 * seed + 10 * c + int(10 * noise))
                src, dst, _, _ = T.plane_scene(rng, c, noise)
                idx = np.arange(c)
                wit = []
                H = T.fit(src, dst, idx, witness=wit)
                cases += 1
                ev = np.sort(wit[0])
                if not ev[1] >= WITNESS * ev[-1]:
                    left_out += 1
                    continue
                assert H is not None and abs(np.linalg.norm(H) - 1.0) < 1e-12 and H[8] >= 0.0
                diff = float(np.max(np.abs(T.unit_sign(H) - T.fit_plain(src, dst, idx))))
                worst = max(worst, diff)
                assert diff <= TOL, (c, noise, seed, diff)
    print(f"twin against SVD: {cases} cases, {left_out} left out by the witness, largest difference {worst:.3g}")
    assert cases == len(SIZES) * len(NOISES) * len(SEEDS)
    assert left_out <= MAX_LEFT_OUT * cases, (left_out, cases)


def test_noise_free_fit_recovers_the_plane(oracle):
    rng = np.random.default_rng(11)
    src, dst, H_true, _ = T.plane_scene(rng, 300, 0.0)
    H = T.fit(src, dst, np.arange(300))
    assert np.max(np.abs(T.unit_sign(H) - H_true)) <= TOL
    assert T.d2_of(src, dst, H).max() < 1e-12


def test_fit_fails_below_four_members_and_on_coincident_points(oracle):
    rng = np.random.default_rng(3)
    src, dst, _, _ = T.plane_scene(rng, 50, 0.5)
    for c in (0, 1, 2, 3):
        assert T.fit(src, dst, np.arange(c)) is None
    assert T.fit(src, dst, np.arange(4)) is not None
    # coincident points: dyadic coordinates and a power-of-two count, so that the centroid IS the point (sum and 1.0 / c
    # are exact), the mean distance 0 and the scale infinite.  (A centroid that rounds away from the point by an ulp gives a
    # huge finite scale instead: then the rule goes on, and the round rule drops the result.)
    same = np.tile(np.array([[512.0, 128.0]]), (50, 1))
    assert T.fit(same, dst, np.arange(32)) is None              # first image
    assert T.fit(src, same, np.arange(32)) is None              # second image
    far = src.copy()
    far[7] = [np.inf, 0.0]
    assert T.fit(far, dst, np.arange(50)) is None               # the centroid is infinite, the scale NaN
    # the members decide, not the array: three real members among fifty points
    assert T.fit(src, dst, np.array([3, 17, 40])) is None


def _h(tag, zero=0.0):
    return np.array([float(tag), zero, 0, 0, 1, 0, 0, 0, 1.0])


def test_round_rule_on_hand_made_sequences():
    chain = {1.0: _h(2), 2.0: _h(3), 3.0: _h(4), 4.0: _h(5)}
    counts = {1.0: 10, 2.0: 12, 3.0: 12, 4.0: 11, 5.0: 50}
    fit_of, count_of = (lambda h: chain.get(h[0])), (lambda h: counts[h[0]])
    # 10 -> 12 accepted, 12 -> 12 accepted (at least as many), 12 -> 11 dropped although 50 waits behind it
    for it, (tag, acc, why) in {0: (1, 0, "iterations"), 1: (2, 1, "iterations"), 2: (3, 2, "iterations"),
                                3: (3, 2, "fewer inliers"), 16: (3, 2, "fewer inliers")}.items():
        H, accepted, reason = T.rounds(_h(1), it, fit_of, count_of)
        assert (H[0], accepted, reason) == (tag, acc, why), it
    # a fit that fails ends the rounds with what stands
    H, accepted, reason = T.rounds(_h(4), 5, lambda h: chain.get(h[0]) if h[0] < 5 else None, lambda h: 1)
    assert (H[0], accepted, reason) == (5.0, 1, "fit failed")
    H, accepted, reason = T.rounds(_h(9), 5, lambda h: None, lambda h: 1)
    assert T.same_bits(H, _h(9)) and (accepted, reason) == (0, "fit failed")
    # a fixed point: the candidate has the bits of what stands, nothing is counted again
    counted = []
    H, accepted, reason = T.rounds(_h(1), 5, lambda h: _h(2), lambda h: counted.append(h[0]) or 7)
    assert (H[0], accepted, reason) == (2.0, 1, "same bits") and counted == [1.0, 2.0]
    # ... bits, not values: -0.0 is another model than 0.0 and goes through the count
    H, accepted, reason = T.rounds(_h(1), 1, lambda h: _h(1, zero=-0.0), lambda h: 7)
    assert accepted == 1 and reason == "iterations" and np.signbit(H[1])
    # H_in comes back as it came, not renormalised
    H_in = 3.0 * _h(1)
    assert T.same_bits(T.rounds(H_in, 4, lambda h: None, lambda h: 0)[0], H_in)


def test_twin_rounds_on_a_scene(oracle):
    """The twin end to end on a small scene: a 4-point hypothesis of a noisy plane gains inliers, never loses any."""
    rng = np.random.default_rng(5)
    src, dst, _, good = T.plane_scene(rng, 400, 1.0, outliers=170)
    H0 = T.fit(src, dst, np.flatnonzero(good)[:4])
    thr2 = 2.2 * 2.2
    got = [T.refit(src, dst, H0, thr2, it) for it in range(5)]
    assert T.same_bits(got[0][0], H0) and got[0][3] == 0
    for it in range(1, 5):
        H, mask, inl, acc = got[it]
        assert inl >= got[it - 1][2] and acc <= it and inl == int(mask.sum())
        assert np.array_equal(mask.astype(bool), T.inlier_mask(src, dst, H, thr2))
    assert got[4][2] > got[0][2]


def test_null_arguments_are_refused(engine_lib):
    """(what can be asked without a device; the parent library lacks the symbol)"""
    H = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    fn = engine_lib.mh_refit_homography
    assert fn(None, H, C.c_double(1.0), 1, H, None, None, None) == -2


def test_header_binding_and_host_hook(mh, engine_lib):
    text = open(os.path.join(ROOT, "include", "multih_hip.h")).read()
    assert re.search(r"MH_API int mh_refit_homography\(mh_engine\* e, const double H_in\[9\], double thr2, int iterations,", text)
    assert "mh_refit_homography" in mh.capi.SYMBOLS and hasattr(mh.Engine, "refit_homography")
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    assert hasattr(host, "mhh_set_tail_refit")


def test_product_library_carries_the_refit_kernel(mh, engine_lib):
    raw = subprocess.run(["strings", mh.LIB_PATH], capture_output=True, text=True).stdout
    names = sorted({l for l in raw.splitlines() if re.match(r"^_ZN2mh\d+k_refit_h", l)})
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    assert sorted({re.sub(r"\(.*", "", d).replace("void ", "") for d in dem}) == ["mh::k_refit_h"], dem
