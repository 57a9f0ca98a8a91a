"""The distance-weighted smoothness (include/multih_hip.h, mh_set_smoothness_weights) without a GPU: the properties of the numpy
twin of the rule (tests/smooth_weights_numpy.py), its repeated-hit form of a weighted graph against the oracle's own folding,
the oracle's alpha-expansion against the reference's GCO on such a graph, the interface (header, binding, export table) and
what MultiH::PlanRun makes of SetSmoothnessWeights (tests/smooth_plan_caller.cpp).  Every comparison is in exact integers."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import expand_tables as X
import smooth_weights_numpy as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "multi-h_amd", "host")
F32_MAX = float(np.finfo(np.float32).max)


def _q(d, rho, q_max):
    return S.quotient(np.asarray(d, np.float32), rho, q_max)


def test_quotient_properties():
    rng = np.random.default_rng(1)
    d = np.sort(np.concatenate([[0.0], 10.0 ** rng.uniform(-3, 12, size=20000), [F32_MAX]]).astype(np.float32))
    for rho, q_max in [(40.0, 8), (0.5, 256), (1000.0, 16), (3.0, 2), (40.0, 1), (1e6, 256)]:
        q = _q(d, rho, q_max)
        assert q[0] == q_max                                        # d == 0
        assert (np.diff(q) <= 0).all()                              # never rises with d
        assert q.min() >= 1 and q.max() <= q_max
        if q_max == 1:
            assert (q == 1).all()
    assert _q([np.inf, np.nan, -np.nan], 40.0, 8).tolist() == [1, 1, 1]
    assert _q([np.inf, np.nan], 1e-200, 256).tolist() == [1, 1]


def test_hand_computed_values():
    # rho = 40: r2 = 1600.  d = 1600 -> t = 1/2: qf = 4 at q_max 8, and exactly 3.5 (a half, away from zero: 4) at q_max 7,
    # 2.5 -> 3 at q_max 5, 0.5 -> 1 (below 1) at q_max 1
    assert _q([1600.0], 40.0, 8).tolist() == [4]
    assert _q([1600.0], 40.0, 7).tolist() == [4]
    assert _q([1600.0], 40.0, 5).tolist() == [3]
    assert _q([1600.0], 40.0, 1).tolist() == [1]
    # d = 4800 -> t = 1/4: 2 at q_max 8, 1.5 -> 2 at q_max 6, 2.5 -> 3 at q_max 10; d = 400 -> t = 0.8: 6.4 -> 6
    assert _q([4800.0, 4800.0 - 1.0, 4800.0 + 1.0], 40.0, 6).tolist() == [2, 2, 1]
    assert _q([4800.0], 40.0, 10).tolist() == [3]
    assert _q([400.0], 40.0, 8).tolist() == [6]
    # far away: 8 * 1600 / (1600 + 11201) = 0.99992... -> 1 by the `>= 1.0` branch; 8 * 1600 / 12800 = 1.0 exactly -> 1
    assert _q([11201.0, 11200.0, 1e30], 40.0, 8).tolist() == [1, 1, 1]
    # the float32 distance itself: (3, 4, 12, 84) -> 9 + 16 + 144 + 7056 = 7225 exactly; q = round(16 * 2500 / 9725) = round(4.113) = 4
    src, dst = np.array([[0.0, 0.0], [3.0, 4.0]]), np.array([[0.0, 0.0], [12.0, 84.0]])
    d = S.distance32(src, dst, [0, 1], [1, 0])
    assert d.dtype == np.float32 and d.tolist() == [7225.0, 7225.0]
    assert _q(d, 50.0, 16).tolist() == [4, 4]
    # coordinates are cast to float32 first: 2^24 + 1 is 2^24 there
    src = np.array([[2.0 ** 24 + 1.0, 0.0], [2.0 ** 24, 0.0]])
    assert S.distance32(src, np.zeros((2, 2)), [0], [1]).tolist() == [0.0]
    # a distance that overflows float32 is infinite, an inf - inf coordinate difference is NaN: both weigh 1
    src = np.array([[3e38, 0.0], [-3e38, 0.0], [1e300, 0.0], [1e300, 0.0]])
    d = S.distance32(src, np.zeros((4, 2)), [0, 2], [1, 3])
    assert np.isinf(d[0]) and np.isnan(d[1])
    assert _q(d, 40.0, 8).tolist() == [1, 1]


def _scene_graph(n, k, seed):
    src, dst, H = S.two_planes(n, seed)
    hit_rp, hit_col = S.knn_hits(src, dst, k)
    return src, dst, H, hit_rp, hit_col


def test_weights_are_symmetric_and_fold_back(oracle):
    src, dst, H, hit_rp, hit_col = _scene_graph(600, 6, 3)
    rp, cl, mult = oracle.build_sym_graph(600, hit_rp, hit_col)
    assert mult.max() == 2 and mult.min() == 1
    w = S.arc_weights(src, dst, rp, cl, mult, S.CAUCHY, 40.0, 8)
    rows = np.repeat(np.arange(600), np.diff(rp))
    # w[k] == w[rev[k]]: the arc (j, i) carries the weight of (i, j)
    key = {(int(i), int(j)): int(x) for i, j, x in zip(rows, cl, w)}
    assert all(key[(j, i)] == x for (i, j), x in key.items())
    assert set(np.unique(w // mult).tolist()) == set(range(1, 9)), "the scene should use every quotient of 1..8"
    assert np.array_equal(S.arc_weights(src, dst, rp, cl, mult, S.CAUCHY, 40.0, 1), mult)
    assert np.array_equal(S.arc_weights(src, dst, rp, cl, mult, S.UNIFORM), mult)
    # the repeated-hit list folds back to the same structure and exactly these weights
    wrp, wcol = S.weighted_hits(rp, cl, w)
    assert wrp[-1] == int(w.sum()) // 2
    rp2, cl2, w2 = oracle.build_sym_graph(600, wrp, wcol)
    assert np.array_equal(rp2, rp) and np.array_equal(cl2, cl) and np.array_equal(w2, w)
    assert S.row_sums(rp, w).tolist() == [int(w[rp[i]:rp[i + 1]].sum()) for i in range(600)]


@pytest.mark.parametrize("n,k,q_max,L", [(600, 6, 8, 5), (2000, 8, 16, 17)])
def test_oracle_expand_equals_reference_gco_on_the_weighted_graph(oracle, n, k, q_max, L):
    src, dst, H, hit_rp, hit_col = _scene_graph(n, k, 3)
    rng = np.random.default_rng(n)
    while H.shape[0] < L - 1:
        H = np.concatenate([H, H[rng.integers(0, 2)][None] * (1 + 3e-4 * rng.normal(size=(1, 9)))])
    rp, cl, mult = oracle.build_sym_graph(n, hit_rp, hit_col)
    w = S.arc_weights(src, dst, rp, cl, mult, S.CAUCHY, 40.0, q_max)
    wrp, wcol = S.weighted_hits(rp, cl, w)
    cost = oracle.data_cost(src, dst, H[:L - 1], 0.5, 2.2 ** 2)
    assert cost.shape == (n, L)
    p = X.Problem(f"cauchy-n{n}", cost, wrp, wcol, oracle.potts(0.5), None)
    assert X.gco_neighbour_entries_fit(p)
    assert X.initial_energy_fits(p)
    lab, e, cyc, _ = oracle.expand(p.cost, p.rowptr, p.col, p.potts)
    assert X.energy_np(p.cost, p.rowptr, p.col, p.potts, lab) == e
    lab_u, e_u, _, _ = oracle.expand(cost, hit_rp, hit_col, p.potts)
    assert not np.array_equal(lab, lab_u), "the weights should change the labeling"
    if oracle.ref() is None:
        pytest.skip("oracle/_ref/libmh_ref_gco.so not built (needs the reference's sources)")
    lab_r, e_r = oracle.ref_expand_table(p.cost, p.rowptr, p.col, p.potts)
    assert e_r == e and np.array_equal(lab_r, lab)


def test_interface_in_step(mh, engine_lib):
    header = open(os.path.join(ROOT, "include", "multih_hip.h")).read()
    assert re.search(r"MH_API\s+int\s+mh_set_smoothness_weights\s*\(\s*mh_engine\s*\*\s*e\s*,\s*int\s+rule\s*,\s*double\s+rho\s*,\s*int\s+q_max\s*\)\s*;", header)
    assert re.search(r"MH_API\s+int\s+mh_get_sym_multiplicity\s*\(\s*mh_engine\s*\*\s*e\s*,\s*int\s*\*\s*mult", header)
    assert re.search(r"#define\s+MH_SMOOTH_UNIFORM\s+0\b", header) and re.search(r"#define\s+MH_SMOOTH_CAUCHY\s+1\b", header)
    assert re.search(r"#define\s+MH_ABI_VERSION\s+2\b", header)
    assert "lambda / sqrt(q_max)" in header and "q_max * round(100*lambda)" in header
    assert mh.capi.SMOOTH_RULES == {"uniform": S.UNIFORM, "cauchy": S.CAUCHY}
    for s in ("mh_set_smoothness_weights", "mh_get_sym_multiplicity"):
        assert s in mh.SYMBOLS and hasattr(engine_lib, s)
    assert hasattr(mh.Engine, "set_smoothness_weights") and hasattr(mh.Engine, "sym_multiplicity")
    # a null engine is refused before anything touches a device
    import ctypes as C
    assert engine_lib.mh_set_smoothness_weights(None, 1, C.c_double(40.0), 8) == -2
    assert engine_lib.mh_set_smoothness_weights(None, 0, C.c_double(0.0), 0) == -2
    assert engine_lib.mh_get_sym_multiplicity(None, None) == -2


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_plan_run_checks_the_smoothness_setting(tmp_path):
    srcs = [os.path.join(ROOT, "tests", "smooth_plan_caller.cpp"), os.path.join(ROOT, "tests", "fake_engine.cpp"),
            *importlib.import_module("multi-h_amd.build").HOST_SOURCES]
    exe = str(tmp_path / "caller")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-ffp-contract=off", "-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                        *srcs, "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "FAILED" not in r.stdout
    m = re.search(r"smooth_plan_caller ok: (\d+) checks", r.stdout)
    assert m and int(m.group(1)) >= 20, r.stdout[-500:]
    assert r.stderr == "", "PlanRun prints nothing"
