"""mh_label_residual_quantile and mh_reweight_homographies_auto without a GPU: the numpy twin of the rules in
include/multih_hip.h (tests/label_scale_numpy.py) held to numpy.partition, to the fixed-scale twin where the bounds coincide, and
to what the data-driven scale is for — a fit that follows the noise of its own label —; and the ABI's pieces (header, binding,
export, host hooks, harness).  tests/test_gpu_label_scale.py holds the kernels to the twin."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import label_scale_numpy as L
import refit_h_numpy as R
import reweight_h_numpy as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MIN = 2.2250738585072014e-308
RANKS = ((0, 1), (1, 2), (3, 4), (1, 1), (65535, 65536))
# shifted_plane seeds at which the cases are what they claim (found with the twin; asserted below)
SEEDS = (0, 1, 2)
FIXED_C2 = 2.5 * 2.5


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _members(c, kind):
    """c members of one plane among 30 % others: (src, dst, labels, H).  kind "runs": the targets are rounded to whole pixels
    under a whole-number translation, so the keys are small whole numbers with long runs of equal ones; "nan": one member's
    error is a NaN (its source is at infinity), which counts as +inf."""
    rng = np.random.default_rng(1000 + c)
    others = max(int(0.3 * c), 1)
    src, dst, H_true, good = R.plane_scene(rng, c, 0.5, outliers=others)
    labels = np.where(good, 0, -1).astype(np.int32)
    H = H_true
    if kind == "runs":
        src = np.round(src)
        dst = src + np.array([5.0, -3.0]) + rng.integers(-2, 3, size=src.shape)
        H = np.array([1.0, 0, 5.0, 0, 1.0, -3.0, 0, 0, 1.0])
    elif kind == "nan":
        src = src.copy()
        src[np.flatnonzero(good)[c // 2]] = np.inf
    return np.ascontiguousarray(src), np.ascontiguousarray(dst), labels, H


@pytest.mark.parametrize("kind", ["plain", "runs", "nan"])
@pytest.mark.parametrize("c", [1, 2, 3, 256, 257])
def test_quantile_against_numpy_partition(c, kind):
    src, dst, labels, H = _members(c, kind)
    idx = np.flatnonzero(labels == 0)
    assert idx.size == c
    with np.errstate(all="ignore"):
        d2 = R.d2_of(src[idx], dst[idx], H)
    if kind == "nan":
        assert np.isnan(d2).sum() == 1
    if kind == "runs" and c >= 256:
        assert np.unique(d2).size <= 13, "whole-number displacements of at most 2 px: at most 13 distinct keys"
    keys = np.where(np.isnan(d2), np.inf, d2)
    for num, den in RANKS:
        r = ((c - 1) * num) // den
        assert 0 <= r < c and (num != 0 or r == 0) and (num != den or r == c - 1)
        want = np.partition(keys, r)[r]
        got, info = L.quantile(src, dst, labels, np.stack([H, H]), num, den)
        assert _bits(got[0]) == _bits(want), (c, num, den, got[0], want)
        assert info[0].tolist() == [c, r, int((keys < want).sum()), 0]
        assert info[0, 2] <= r and (keys <= want).sum() > r, "the rank falls inside the run of the value"
        assert info[1].tolist() == [0, 0, 0, 1] and _bits(got[1]) == L.QNAN_BITS
    if kind == "nan":
        assert np.isinf(L.quantile(src, dst, labels, H, 1, 1)[0][0])
        if c > 1:
            assert np.isfinite(L.quantile(src, dst, labels, H, 65535, 65536)[0][0])


def test_rank_rule():
    assert [L.rank_of(c, 1, 2) for c in (1, 2, 3, 4, 5)] == [0, 0, 1, 1, 2], "the lower median"
    assert L.rank_of(65536, 65535, 65536) == 65534 and L.rank_of(2 ** 31 - 1, 65536, 65536) == 2 ** 31 - 2


@pytest.mark.parametrize("c", [4, 5, 255, 257, 513])
def test_equal_bounds_give_the_fixed_scale_twin_bit_for_bit(c):
    rng = np.random.default_rng(300 + c)
    others = max(int(0.3 * c), 1)
    src, dst, H_true, good = R.plane_scene(rng, c, 0.5, outliers=others)
    labels = np.where(good, 0, np.where(rng.random(c + others) < 0.5, 1, -1)).astype(np.int32)
    H0 = H_true / H_true[8]
    H0[2] += 0.8
    H_nan = H0.copy()
    H_nan[3] = np.nan
    H_in = np.stack([H0, np.eye(3).reshape(9), H_nan, H0])               # label 2: status 2 or 1; label 3: nobody
    c2 = 2.2 * 2.2
    for rounds in (0, 1, 3):
        H, gain, info = W.reweight(src, dst, labels, H_in, c2, rounds)
        for num, den, kappa2 in ((1, 2, L.KAPPA2_DEFAULT), (0, 1, 1e-300), (1, 1, 1e300)):
            Ha, ga, sa, ia = L.reweight_auto(src, dst, labels, H_in, num, den, kappa2, c2, c2, rounds)
            assert np.array_equal(_bits(Ha), _bits(H)) and np.array_equal(_bits(ga), _bits(gain)) and np.array_equal(ia, info)
            assert np.all(sa[info[:, 3] == 0] == c2) and np.all(sa[info[:, 3] != 0] == 0.0)


def _case(sigma, contaminants, seed):
    src, dst, H_true, on_plane = L.shifted_plane(np.random.default_rng(seed), sigma, contaminants)
    n = src.shape[0]
    plane = np.flatnonzero(on_plane)
    assert plane.size == 400 and n == 400 + contaminants
    H0 = R.fit(src, dst, np.arange(n))
    labels = np.zeros(n, np.int32)
    rms = lambda H: W.rms_to_truth(src, H, H_true, plane) / sigma
    fixed = W.reweight(src, dst, labels, H0, FIXED_C2, 3)[0][0]
    auto, gain, scale, info = L.reweight_auto(src, dst, labels, H0, 1, 2, L.KAPPA2_DEFAULT, DBL_MIN, 1e6, 3)
    assert tuple(info[0, [0, 2, 3]]) == (n, 3, 0)
    return rms(H0), rms(fixed), rms(auto[0]), float(np.sqrt(scale[0, 1])) / sigma


@pytest.mark.parametrize("seed", SEEDS)
def test_small_noise_with_contaminants_where_the_fixed_scale_removes_nothing(seed):
    """sigma = 0.1 px, 40 contaminants 0.5 px to one side: c = 2.5 px keeps them all with nearly full weight; the label's own
    median does not.  Three auto rounds end nearer the truth than the plain fit and than three rounds at the fixed scale.
    (The twin gave, in units of sigma, plain 0.41-0.46, fixed 0.40-0.45, auto 0.14-0.19 at these seeds.)"""
    plain, fixed, auto, scale = _case(0.1, 40, seed)
    print(f"seed {seed}: RMS to the truth / sigma: plain {plain:.3f}, fixed {fixed:.3f}, auto {auto:.3f}; scale {scale:.2f} sigma")
    assert fixed > 0.9 * plain, "premise: the fixed scale removes next to nothing"
    assert auto < plain and auto < fixed
    assert 2.0 < scale < 4.0


@pytest.mark.parametrize("seed", SEEDS)
def test_large_noise_on_a_clean_set_where_the_fixed_scale_cuts_into_the_noise(seed):
    """sigma = 1.5 px, no contaminants: c = 2.5 px is 1.67 sigma and discards a quarter of a clean set; the auto scale stays
    near 3 sigma.  (The twin gave plain 0.15-0.17, fixed 0.21-0.37, auto 0.14-0.21.)"""
    plain, fixed, auto, scale = _case(1.5, 0, seed)
    print(f"seed {seed}: RMS to the truth / sigma: plain {plain:.3f}, fixed {fixed:.3f}, auto {auto:.3f}; scale {scale:.2f} sigma")
    assert fixed > plain, "premise: the fixed scale damages the clean set"
    assert auto < fixed
    assert 2.0 < scale < 4.0


@pytest.mark.parametrize("seed", SEEDS)
def test_the_scale_follows_the_noise_at_the_matching_level_too(seed):
    """sigma = 0.5 px, 40 contaminants: the scale under the final model between 2 and 4 sigma here as at the other two levels
    (the twin gave 2.87-3.46 sigma over eight seeds and all three levels), and the fit nearer the truth than the plain one."""
    plain, fixed, auto, scale = _case(0.5, 40, seed)
    print(f"seed {seed}: RMS to the truth / sigma: plain {plain:.3f}, fixed {fixed:.3f}, auto {auto:.3f}; scale {scale:.2f} sigma")
    assert auto < plain
    assert 2.0 < scale < 4.0


def test_clamps_statuses_and_the_zero_median():
    rng = np.random.default_rng(5)
    src, dst, H_true, good = R.plane_scene(rng, 300, 0.5, outliers=90)
    labels = np.where(good, 0, -1).astype(np.int32)
    labels[np.flatnonzero(~good)[:3]] = 1
    H_in = np.stack([H_true, H_true, H_true])
    q = L.quantile(src, dst, labels, H_in, 1, 2)[0][0]
    for lo, hi, want in ((4.0 * q, 8.0 * q, 4.0 * q), (q / 8, q / 4, q / 4), (2.0 * q, 3.0 * q, 2.0 * q), (q, 2.0 * q, 2.0 * q)):
        H, gain, scale, info = L.reweight_auto(src, dst, labels, H_in, 1, 2, 2.0, lo, hi, 0)
        assert scale[0, 0] == scale[0, 1] == want and info[:, 3].tolist() == [0, 1, 1] and np.all(scale[1:] == 0.0)
        assert R.same_bits(H, H_in) and gain[0, 0] == gain[0, 1] > 0
    # at least half the members fit exactly: the median is 0, c2 = c2_min, only the exact fits weigh (each 1.0)
    src = rng.integers(0, 1000, size=(40, 2)).astype(np.float64)
    dst = src + np.array([5.0, -3.0])
    dst[25:] += rng.normal(0, 0.4, size=(15, 2))
    Ht = np.array([1.0, 0, 5.0, 0, 1.0, -3.0, 0, 0, 1.0])
    H, gain, scale, info = L.reweight_auto(src, dst, np.zeros(40, np.int32), Ht, 1, 2, L.KAPPA2_DEFAULT, DBL_MIN, 24.5, 0)
    assert tuple(scale[0]) == (DBL_MIN, DBL_MIN) and tuple(info[0]) == (40, 25, 0, 0) and tuple(gain[0]) == (25.0, 25.0)
    H, gain, scale, info = L.reweight_auto(src, dst, np.zeros(40, np.int32), Ht, 1, 2, L.KAPPA2_DEFAULT, DBL_MIN, 24.5, 3)
    assert scale[0, 0] == DBL_MIN and gain[0, 0] == 25.0 and info[0, 3] == 0 and info[0, 2] >= 1
    assert W.rms_to_truth(src, H[0], Ht, np.arange(25)) < 1e-9, "the fit of the exact members alone"


def test_header_binding_and_host_hooks(mh, engine_lib):
    text = open(os.path.join(ROOT, "include", "multih_hip.h")).read()
    assert "#define MH_QUANTILE_MAX_DEN 65536" in text
    assert re.search(r"MH_API int mh_label_residual_quantile\(mh_engine\* e, const int\* labels /\* n \*/, const double\* H /\* m x 9 \*/, int m,\s+"
                     r"int num, int den, double\* d2_out /\* m \*/,", text)
    assert re.search(r"MH_API int mh_reweight_homographies_auto\(mh_engine\* e, const int\* labels /\* n \*/, const double\* H_in /\* m x 9 \*/, int m,\s+"
                     r"int num, int den, double kappa2, double c2_min, double c2_max, int rounds,", text)
    assert ("MH_API int mh_set_estimator_reweighting_auto(mh_engine* e, int rounds, int num, int den, double kappa2, double c2_min, "
            "double c2_max);") in text
    assert "NOT comparable" in text, "the header says that the two W of gain belong to different scales"
    for name in ("mh_label_residual_quantile", "mh_reweight_homographies_auto", "mh_set_estimator_reweighting_auto"):
        assert name in mh.capi.SYMBOLS and hasattr(engine_lib, name)
    for name in ("label_residual_quantile", "reweight_homographies_auto", "set_estimator_reweighting_auto"):
        assert hasattr(mh.Engine, name)
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    assert hasattr(host, "mhh_set_model_reweight_auto") and hasattr(host, "mhh_set_estimator_reweight_auto")


def test_the_harness_refuses_auto_reweighting_arguments_out_of_range(mh, engine_lib, tmp_path):
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    assert os.path.exists(harness), "harness not built"
    run = lambda *opts: subprocess.run([harness, str(tmp_path / "in.txt"), str(tmp_path / "out.txt"), *opts],
                                       capture_output=True, text=True, timeout=60)
    for opt in ("--reweight-auto", "--estimator-reweight-auto"):
        for bad in ("17", "-1", "x", "", "3:", "3:0", "3:-2", "3:x", "3:2.5k", ":2.5", "3:inf", "3:nan"):
            r = run(opt, bad)
            assert r.returncode == 2 and opt in r.stderr and "[0, 16]" in r.stderr, (opt, bad, r.returncode, r.stderr)
        for good in ("0", "3", "16:2.5"):                                    # accepted: the run then ends on the missing input file
            r = run(opt, good)
            assert r.returncode != 2 and "[0, 16]" not in r.stderr, (opt, good, r.returncode, r.stderr)
    for base in ("--reweight", "--estimator-reweight"):
        r = run(base, "2", base + "-auto", "3")
        assert r.returncode == 2 and base + "-auto" in r.stderr, (base, r.returncode, r.stderr)
        r = run(base + "-auto", "3:2", base, "1:2.2")
        assert r.returncode == 2, (base, r.returncode, r.stderr)
        for a, b in (("0", "3"), ("2", "0")):                                # one of the two off: accepted
            r = run(base, a, base + "-auto", b)
            assert r.returncode != 2, (base, a, b, r.returncode, r.stderr)


def test_product_library_carries_the_two_kernels(mh, engine_lib):
    raw = subprocess.run(["strings", mh.LIB_PATH], capture_output=True, text=True).stdout
    names = sorted({l for l in raw.splitlines() if re.match(r"^_ZN2mh\d+k_(label_quantile|autoscale_reweight_h)", l)})
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    assert sorted({re.sub(r"\(.*", "", d).replace("void ", "") for d in dem}) == ["mh::k_autoscale_reweight_h", "mh::k_label_quantile"], dem
