"""mh_reweight_homographies without a GPU: the numpy twin of the rule in include/multih_hip.h (tests/reweight_h_numpy.py) held to
the plain definition of a weighted fit, to the unweighted fit it reduces to at unit weights, and to what it is for — a model
nearer the truth on a contaminated label set —; and the ABI's pieces (header, binding, export, host hooks).
tests/test_gpu_reweight_h.py holds the kernel to the twin."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import refit_h_numpy as R
import reweight_h_numpy as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-6                         # the project's tolerance for homographies (unit norm, sign fixed): tests/test_reestimate_dlt_cpu.py
C2 = 2.2 * 2.2
COUNTS = (4, 5, 255, 256, 257, 513, 2000)
# contaminated_plane seeds at which the case is what it claims (found with the twin; asserted below)
CONTAMINATED_SEEDS = (11, 12, 13)


def _scattered(rng, c, noise=0.5):
    """c members of one plane at scattered ascending point indices among 30 % others: (src, dst, idx, H_true)."""
    others = max(int(0.3 * c), 1)
    src, dst, H_true, good = R.plane_scene(rng, c, noise, outliers=others)
    return src, dst, np.flatnonzero(good), H_true


@pytest.mark.parametrize("c", COUNTS)
def test_twin_equals_the_plain_definition(c):
    """One weighted fit on random weights in (0, 1], with a fifth of them exactly 0 where that leaves at least four."""
    rng = np.random.default_rng(100 + c)
    src, dst, idx, _ = _scattered(rng, c)
    w = rng.uniform(0.05, 1.0, size=c)
    if c >= 255:
        w[rng.choice(c, c // 5, replace=False)] = 0.0
    twin = W.wfit(src, dst, idx, w)
    plain = W.wfit_plain(src, dst, idx, w)
    err = np.abs(R.unit_sign(twin) - plain).max()
    print(f"members {c}: |twin - eigh| = {err:.3e}")
    assert err <= TOL, (c, err)


@pytest.mark.parametrize("seed", CONTAMINATED_SEEDS)
def test_twin_equals_the_plain_definition_on_the_contaminated_scene(seed):
    """Every round's fit of a three-round run, with the weights the rule gives."""
    src, dst, H_true, on_plane = W.contaminated_plane(np.random.default_rng(seed))
    idx = np.arange(src.shape[0])
    cur = R.fit(src, dst, idx)
    for r in range(3):
        w = W.weights(src, dst, idx, cur, C2)
        assert 4 <= int((w > 0).sum()) < idx.size or r == 0
        twin = W.wfit(src, dst, idx, w)
        err = np.abs(R.unit_sign(twin) - W.wfit_plain(src, dst, idx, w)).max()
        print(f"seed {seed} round {r + 1}: |twin - eigh| = {err:.3e}")
        assert err <= TOL, (seed, r, err)
        cur = twin


@pytest.mark.parametrize("c", COUNTS)
def test_unit_weights_give_the_unweighted_fit_bit_for_bit(c):
    rng = np.random.default_rng(200 + c)
    src, dst, idx, _ = _scattered(rng, c)
    assert R.same_bits(W.wfit(src, dst, idx, np.ones(c)), R.fit(src, dst, idx))


@pytest.mark.parametrize("seed", CONTAMINATED_SEEDS)
def test_three_rounds_bring_a_contaminated_model_nearer_the_truth(seed):
    """400 members of a plane at 0.5 px noise and 40 displaced about 2.5 px to one side, c2 = 2.2^2: after three rounds from the
    unweighted fit the model lies strictly nearer the true homography over the plane's points.  The direction only."""
    src, dst, H_true, on_plane = W.contaminated_plane(np.random.default_rng(seed))
    n = src.shape[0]
    labels = np.zeros(n, dtype=np.int32)
    plane = np.flatnonzero(on_plane)
    assert plane.size == 400 and n == 440
    off = np.linalg.norm(dst[~on_plane] - _carried(src, H_true)[~on_plane], axis=1)
    assert 1.5 < off.mean() < 3.5, "the contaminants should lie about 2.5 px off the plane"
    H0 = R.fit(src, dst, np.arange(n))
    H, gain, info = W.reweight(src, dst, labels, H0, C2, 3)
    assert tuple(info[0, [0, 2, 3]]) == (n, 3, 0) and info[0, 1] < n, "three rounds, and some member is outside c2"
    before, after = W.rms_to_truth(src, H0, H_true, plane), W.rms_to_truth(src, H[0], H_true, plane)
    print(f"seed {seed}: RMS to the truth {before:.4f} px unweighted, {after:.4f} px after three rounds")
    assert after < before


def _carried(src, H):
    q = np.concatenate([src, np.ones((src.shape[0], 1))], axis=1) @ np.asarray(H).reshape(3, 3).T
    return q[:, :2] / q[:, 2:3]


def test_rounds_statuses_and_the_round_rule():
    rng = np.random.default_rng(7)
    src, dst, H_true, good = R.plane_scene(rng, 300, 0.5, outliers=90)
    labels = np.where(good, 0, -1).astype(np.int32)
    labels[np.flatnonzero(~good)[:3]] = 1                                    # label 1: three members; label 2: none
    H_nan = H_true.copy()
    H_nan[4] = np.nan
    H_in = np.stack([H_true, H_true, H_true])
    H, gain, info = W.reweight(src, dst, labels, H_in, C2, 0)
    assert info.tolist() == [[300, info[0, 1], 0, 0], [3, 0, 0, 1], [0, 0, 0, 1]] and gain[0, 0] == gain[0, 1] > 0
    assert R.same_bits(H, H_in) and np.all(gain[1:] == 0.0)
    H, gain, info = W.reweight(src, dst, labels, np.stack([H_nan, H_nan, H_true]), C2, 3)
    assert info[:, 3].tolist() == [2, 1, 1] and R.same_bits(H[0], H_nan) and np.all(gain == 0.0)
    # a model with no member inside c2
    far = H_true.copy()
    far[2] += 500.0 * far[8]
    H, gain, info = W.reweight(src, dst, labels, np.stack([far, H_true, H_true]), C2, 3)
    assert tuple(info[0]) == (300, 0, 0, 0) and R.same_bits(H[0], far) and tuple(gain[0]) == (0.0, 0.0)
    # exact data: the fit of a fit reproduces itself and the rounds stop early
    src2, dst2, H2, _ = R.plane_scene(np.random.default_rng(8), 300, 0.0)
    one = W.reweight(src2, dst2, np.zeros(300, np.int32), H2, C2, 1)[0][0]
    H, gain, info = W.reweight(src2, dst2, np.zeros(300, np.int32), one, C2, 16)
    assert info[0, 2] < 16 and info[0, 1] == 300


def test_header_binding_and_host_hooks(mh, engine_lib):
    text = open(os.path.join(ROOT, "include", "multih_hip.h")).read()
    assert "#define MH_REWEIGHT_MAX_ROUNDS 16" in text
    assert re.search(r"MH_API int mh_reweight_homographies\(mh_engine\* e, const int\* labels /\* n \*/, const double\* H_in /\* m x 9 \*/, int m,\s+"
                     r"double c2, int rounds, double\* H_out /\* m x 9 \*/,", text)
    assert "MH_API int mh_set_estimator_reweighting(mh_engine* e, int rounds, double c2);" in text
    for name in ("mh_reweight_homographies", "mh_set_estimator_reweighting"):
        assert name in mh.capi.SYMBOLS and hasattr(engine_lib, name)
    assert hasattr(mh.Engine, "reweight_homographies") and hasattr(mh.Engine, "set_estimator_reweighting")
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    assert hasattr(host, "mhh_set_model_reweight") and hasattr(host, "mhh_set_estimator_reweight")


def test_the_harness_refuses_reweighting_arguments_out_of_range(mh, engine_lib, tmp_path):
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    assert os.path.exists(harness), "harness not built"
    for opt in ("--reweight", "--estimator-reweight"):
        for bad in ("17", "-1", "x", "", "3:", "3:0", "3:-2", "3:x", "3:2.2px", ":2.2"):
            r = subprocess.run([harness, str(tmp_path / "in.txt"), str(tmp_path / "out.txt"), opt, bad],
                               capture_output=True, text=True, timeout=60)
            assert r.returncode == 2 and opt in r.stderr and "[0, 16]" in r.stderr, (opt, bad, r.returncode, r.stderr)
        for good in ("0", "3", "16:4.95"):                                   # accepted: the run then ends on the missing input file
            r = subprocess.run([harness, str(tmp_path / "in.txt"), str(tmp_path / "out.txt"), opt, good],
                               capture_output=True, text=True, timeout=60)
            assert r.returncode != 2 and "[0, 16]" not in r.stderr, (opt, good, r.returncode, r.stderr)


def test_product_library_carries_the_reweight_kernel(mh, engine_lib):
    raw = subprocess.run(["strings", mh.LIB_PATH], capture_output=True, text=True).stdout
    names = sorted({l for l in raw.splitlines() if re.match(r"^_ZN2mh\d+k_reweight_h", l)})
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    assert sorted({re.sub(r"\(.*", "", d).replace("void ", "") for d in dem}) == ["mh::k_reweight_h"], dem
