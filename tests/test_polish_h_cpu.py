"""mh_polish_homographies without a GPU: the numpy twin of the rule in include/multih_hip.h (tests/polish_h_numpy.py) held to an
independent definition — scipy's MINPACK Levenberg-Marquardt on the same residuals — and to the rule's own properties, and
the ABI's pieces (header, binding, export, kernel symbol).  tests/test_gpu_polish_h.py holds the kernel to the twin."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import polish_h_numpy as P
import refit_h_numpy as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9                                       # see test_twin_reaches_the_least_squares_optimum


def _residuals(x, src, dst):
    w = x[6] * src[:, 0] + x[7] * src[:, 1] + 1.0
    return np.concatenate([(x[0] * src[:, 0] + x[1] * src[:, 1] + x[2]) / w - dst[:, 0],
                           (x[3] * src[:, 0] + x[4] * src[:, 1] + x[5]) / w - dst[:, 1]])


def _optimum(src, dst, starts):
    """S*: the smallest sum of squares scipy's LM reaches from any of the starts, tolerances at 1e-15."""
    from scipy.optimize import least_squares
    best = np.inf
    for s in starts:
        s = np.asarray(s, np.float64).reshape(9)
        r = least_squares(_residuals, s[:8] / s[8], args=(src, dst), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        best = min(best, float((r.fun ** 2).sum()))
    return best


def _scene(c, seed=0):
    """c members of one plane at 0.5 px noise and a start about a pixel off the truth."""
    rng = np.random.default_rng(1000 * c + seed)
    src, dst, H_true, _ = T.plane_scene(rng, c, 0.5)
    H0 = H_true / H_true[8]
    H0[2] += rng.normal(0, 1.0)
    H0[5] += rng.normal(0, 1.0)
    return src, dst, H_true, H0


@pytest.mark.parametrize("c", [8, 17, 64, 255, 256, 257, 513, 2000])
def test_twin_reaches_the_least_squares_optimum(c):
    """Ten iterations from a start a pixel off end within TOL (relative) of the optimum of scipy.optimize.least_squares
    (method "lm", tolerances 1e-15, the best of three starts: the input, the truth, the twin's own result).  The twin's
    measured worst over these scenes is 3.2e-13 (8 members), below 1e-10, so TOL is 1e-9; the Jacobi works in pixel
    coordinates, no normalisation was needed."""
    src, dst, H_true, H0 = _scene(c)
    H, (S0, S1), (members, it, acc, status) = P.polish_one(src, dst, np.arange(c), H0, 10)
    S_star = _optimum(src, dst, [H0, H_true, H])
    print(f"[polish twin] c={c}: S {S0:.6g} -> {S1:.12g}, S* {S_star:.12g}, rel {S1 / S_star - 1:.3e}, {it} iterations, {acc} accepted")
    assert (members, status) == (c, 0) and acc >= 1 and it <= 10
    assert S1 <= S_star * (1.0 + TOL)
    assert H[8] == 1.0 and abs(P.transfer_error_sum(src, dst, np.arange(c), H) - S1) <= 1e-9 * S1


@pytest.mark.parametrize("c", [5, 6])
def test_small_sets_never_get_worse(c):
    for seed in range(4):
        src, dst, _, H0 = _scene(c, seed)
        H, (S0, S1), info = P.polish_one(src, dst, np.arange(c), H0, 10)
        assert S1 <= S0 and np.all(np.isfinite(H)) and np.isfinite(S0) and np.isfinite(S1) and info[3] == 0


def test_cost_never_rises_and_zero_iterations_return_the_input():
    rng = np.random.default_rng(3)
    src, dst, H_true, good = T.plane_scene(rng, 300, 0.5, outliers=100)
    labels = np.where(good, 0, -1)
    idx = np.flatnonzero(good)
    H4 = T.fit(src, dst, np.sort(rng.choice(idx, 4, replace=False)))
    for H0 in (H_true, 7.0 * H_true, H4, -H4):
        last = None
        for it in (0, 1, 2, 5, 10, 32):
            H, cost, info = P.polish(src, dst, labels, H0, it)
            assert cost[0, 1] <= cost[0, 0] and info[0, 0] == 300 and info[0, 1] <= it and info[0, 2] <= info[0, 1]
            if it == 0:
                assert T.same_bits(H[0], H0) and cost[0, 0] == cost[0, 1] and tuple(info[0]) == (300, 0, 0, 0)
            if last is not None:
                assert cost[0, 1] <= last and cost[0, 0] == first
            first, last = cost[0, 0], cost[0, 1]
        assert abs(P.transfer_error_sum(src, dst, idx, H[0]) - cost[0, 1]) <= 1e-9 * cost[0, 1]


def test_exactly_four_members():
    """Four points fix a homography: from their own DLT fit S is at rounding level, one iteration runs and max |r| ends the loop."""
    for seed in range(4):
        rng = np.random.default_rng(seed)
        src, dst, _, _ = T.plane_scene(rng, 4, 0.5)
        H0 = T.fit(src, dst, np.arange(4))
        H, (S0, S1), info = P.polish_one(src, dst, np.arange(4), H0, 10)
        assert S0 < 1e-18 and S1 <= S0 and info == (4, 1, info[2], 0) and info[2] in (0, 1)
    # three members: status 1, the input's bits
    H, cost, info = P.polish_one(src, dst, np.arange(3), 3.0 * H0, 10)
    assert T.same_bits(H, 3.0 * H0) and cost == (0.0, 0.0) and info == (3, 0, 0, 1)
    # a model without a finite parametrisation: status 2
    for bad in (np.array([1, 0, 0, 0, 1, 0, 0, 0, 0.0]), np.array([1, 0, np.nan, 0, 1, 0, 0, 0, 1.0])):
        H, cost, info = P.polish_one(src, dst, np.arange(4), bad, 10)
        assert T.same_bits(H, bad) and cost == (0.0, 0.0) and info == (4, 0, 0, 2)


def test_restated_jacobi_is_the_oracles(oracle):
    """The twin's Jacobi, restated in numpy, against the C restatement the other twins use: the same bits."""
    rng = np.random.default_rng(11)
    for n in (3, 8, 9):
        B = rng.normal(size=(2 * n, n)) * rng.uniform(1e-3, 1e3, size=n)
        A = B.T @ B
        A = 0.5 * (A + A.T)
        d, V = P.jacobi_sym(A)
        d_o, V_o = oracle.jacobi_sym(A)
        assert T.same_bits(d, d_o) and T.same_bits(V, V_o)
        assert np.max(np.abs(np.sort(d) - np.linalg.eigvalsh(A))) <= 1e-9 * np.max(np.abs(d))


def test_null_arguments_are_refused(engine_lib):
    """(what can be asked without a device; the parent library lacks the symbol)"""
    H = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    lab = (C.c_int * 4)(0, 0, 0, 0)
    fn = engine_lib.mh_polish_homographies
    assert fn(None, lab, H, 1, 1, H, None, None) == -2


def test_header_binding_and_host_hooks(mh, engine_lib):
    text = open(os.path.join(ROOT, "include", "multih_hip.h")).read()
    assert "#define MH_POLISH_MAX_ITERATIONS 32" in text
    assert re.search(r"MH_API int mh_polish_homographies\(mh_engine\* e, const int\* labels /\* n \*/, const double\* H_in /\* m x 9 \*/, int m,",
                     text)
    assert "mh_polish_homographies" in mh.capi.SYMBOLS and hasattr(mh.Engine, "polish_homographies")
    assert hasattr(engine_lib, "mh_polish_homographies")
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    assert hasattr(host, "mhh_set_tail_polish") and hasattr(host, "mhh_set_model_polish")


def test_the_harness_refuses_polish_counts_out_of_range(mh, engine_lib, tmp_path):
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    assert os.path.exists(harness), "harness not built"
    for opt in ("--tail-polish", "--polish"):
        for bad in ("33", "-1", "x", ""):
            r = subprocess.run([harness, str(tmp_path / "in.txt"), str(tmp_path / "out.txt"), opt, bad],
                               capture_output=True, text=True, timeout=60)
            assert r.returncode == 2 and opt in r.stderr and "[0, 32]" in r.stderr, (opt, bad, r.returncode, r.stderr)


def test_product_library_carries_the_polish_kernel(mh, engine_lib):
    raw = subprocess.run(["strings", mh.LIB_PATH], capture_output=True, text=True).stdout
    names = sorted({l for l in raw.splitlines() if re.match(r"^_ZN2mh\d+k_polish_h", l)})
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    assert sorted({re.sub(r"\(.*", "", d).replace("void ", "") for d in dem}) == ["mh::k_polish_h"], dem
