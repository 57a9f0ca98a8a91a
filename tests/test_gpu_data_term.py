"""GPU tests of the selectable data term (mh_set_data_term, include/multih_hip.h) against the numpy twin of
tests/data_term_numpy.py, which tests/test_data_term_cpu.py pins to the oracle under MH_DATA_TERM_REFERENCE.  Every
comparison is exact integer equality (homographies: as the tests they are modelled on say).

The cost tables: k_data_cost, k_cost_matrix (mh_set_tuning key 15 = 0), k_rising32 (key 23 = 0) and k_rising32_resident at the
sizes where each kernel takes another path — lane groups of 4, the 1 024-point tile of k_cost_matrix and its tail, the
32-model block of the pre-test kernel and the 16-model block of k_cost_matrix — with lam = 100 / lambda integer and not, on
models that make d2 = 0, a non-finite d2, d2 within a few ulp of T on either side, and far pairs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import data_term_numpy as T
import test_gpu_alternation as alt

pytestmark = pytest.mark.gpu
THR, LOCALITY = 2.2, 0.005
THR2 = THR * THR
NS = (1, 3, 255, 1024, 1025, 4099)
MS = (1, 31, 32, 33, 65)


def _near_T_offsets():
    """Offsets dx with fl(dx * dx) within a few ulp of T = thr^2 81/16, on both sides of it."""
    Tt = THR2 * 81.0 / 16.0
    dx = [np.sqrt(Tt)]
    for _ in range(4):
        dx.insert(0, np.nextafter(dx[0], 0.0))
        dx.append(np.nextafter(dx[-1], np.inf))
    return np.array(dx), Tt


@pytest.fixture(scope="module")
def pool(synth, oracle):
    """4 099 points and 65 models, and the forward error of every pair (the oracle's, bit-equal to the engine's), once."""
    sc = synth.make_scene(4099, 3, seed=5, with_neighbours=False)
    src, dst = sc.src.copy(), sc.dst.copy()
    dx, Tt = _near_T_offsets()
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
    while len(H) < 65:
        if len(H) % 2:
            H.append(sc.H_true[len(H) % 3] * (1.0 + rng.normal(0, 1e-3, size=9)))       # near a plane: many pairs inside T
        else:
            H.append((np.eye(3) + rng.normal(0, 0.05, size=(3, 3))).reshape(9))          # far from everything
    H = np.ascontiguousarray(np.array(H))
    with np.errstate(all="ignore"):
        d2 = oracle.residual_matrix(src, dst, H)
    ulp = np.spacing(Tt)
    row = d2[0]
    assert ((row < Tt) & (Tt - row <= 8 * ulp)).any() and ((row >= Tt) & (row - Tt <= 8 * ulp)).any(), "near-miss pairs on both sides of T"
    assert (row == 0.0).any() and np.isinf(d2[1]).any() and np.isnan(d2[2]).any()
    assert (d2[3:] < Tt).mean() > 0.02 and (d2[3:] > 100 * Tt).mean() > 0.2
    return src, dst, H, d2


def _set_path(engine, path):
    if path == "fp64":
        engine.set_tuning(15, 0)            # k_cost_matrix, no FP32 pre-test
    elif path == "pretest_plain":
        engine.set_tuning(23, 0)            # k_rising32 by hardware dispatch
    else:
        assert path == "pretest_default"    # the resident grid wherever the items outnumber it (not at these sizes: see the test below)


@pytest.mark.parametrize("lam", [0.5, 0.3])
@pytest.mark.parametrize("path", ["pretest_default", "pretest_plain", "fp64"])
def test_rising_tables_equal_the_twin_and_reference_is_untouched(engine, oracle, pool, path, lam):
    src, dst, H, d2 = pool
    engine.set_params(2.6, THR, LOCALITY, lam, 20)
    _set_path(engine, path)
    rising = T.term_of_d2(d2, lam, THR2, T.RISING)              # [model, point]
    reference = oracle.data_cost(src, dst, H, lam, THR2)        # [point, label]: the parent-defined output
    assert np.array_equal(T.term_of_d2(d2, lam, THR2, T.REFERENCE), reference[:, 1:].T)
    B = T.outlier_cost(lam, THR2)
    inl = d2 < THR2
    for n in NS:
        engine.set_correspondences(src[:n], dst[:n])
        for m in MS:
            engine.set_models(H[:m])
            Cm_ref, cnt_ref = engine.cost_matrix()
            engine.set_data_term("rising")
            Cm, cnt = engine.cost_matrix()
            cost = engine.data_cost()
            engine.set_data_term("reference")
            Cm_back, cnt_back = engine.cost_matrix()
            cost_back = engine.data_cost()
            where = (path, lam, n, m)
            assert np.array_equal(Cm, rising[:m, :n]), where
            assert np.array_equal(cost[:, 1:], Cm.T) and np.all(cost[:, 0] == B), where
            assert np.array_equal(cnt, cnt_ref) and np.array_equal(cnt, inl[:m, :n].sum(axis=1)), where
            # ... and the switch leaks nothing: before and after, the default is the oracle's dataEnergy
            assert np.array_equal(Cm_ref, reference[:n, 1:m + 1].T) and np.array_equal(Cm_back, Cm_ref), where
            assert np.array_equal(cost_back, reference[:n, :m + 1]) and np.array_equal(cnt_back, cnt_ref), where
    assert not np.array_equal(rising, reference[:, 1:].T)


def test_rising_table_on_the_resident_grid(engine, oracle, pool):
    """k_rising32_resident: the resident grid is taken when the work items (32-model blocks x point slices, 8 slices by
    default) outnumber the workgroups the device holds — 2 per compute unit, 512 on 256 compute units — so 66 model blocks
    (the last one a single model) x 8 slices of a 16 389-point set; and the same through the plain launch."""
    src, dst, H, _ = pool
    rng = np.random.default_rng(9)
    n, m = 8 * 2048 + 5, 65 * 32 + 1
    src = np.ascontiguousarray(np.concatenate([src] * 4 + [src[:5]])[:n])
    dst = np.ascontiguousarray(np.concatenate([dst] * 4 + [dst[:5]])[:n] + np.repeat(rng.normal(0, 0.5, size=(5, 2)), 4099, axis=0)[:n])
    Hs = np.ascontiguousarray(np.concatenate([H[:3], np.tile(H[3:], (34, 1))[:m - 3] * (1.0 + rng.normal(0, 2e-4, size=(m - 3, 9)))]))
    engine.set_params(2.6, THR, LOCALITY, 0.3, 20)
    engine.set_correspondences(src, dst)
    engine.set_models(Hs)
    with np.errstate(all="ignore"):
        d2 = oracle.residual_matrix(src, dst, Hs)
    want = T.term_of_d2(d2, 0.3, THR2, T.RISING)
    want_cnt = (d2 < THR2).sum(axis=1)
    assert (d2 < THR2 * 81.0 / 16.0).mean() > 0.01
    engine.set_data_term("rising")
    Cm, cnt = engine.cost_matrix()
    assert np.array_equal(Cm, want) and np.array_equal(cnt, want_cnt)
    engine.set_tuning(23, 0)
    Cm2, cnt2 = engine.cost_matrix()
    assert np.array_equal(Cm2, want) and np.array_equal(cnt2, want_cnt)
    engine.set_data_term("reference")
    Cm3, cnt3 = engine.cost_matrix()
    assert np.array_equal(Cm3, T.term_of_d2(d2, 0.3, THR2, T.REFERENCE)) and np.array_equal(cnt3, want_cnt)


def test_setting_the_term_marks_the_cost_stale_and_bad_values_are_refused(mh, engine, synth):
    sc = synth.make_scene(300, 3, seed=2)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_epipolar(sc.F, sc.e2)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    engine.set_models(sc.H_true)
    engine.data_cost(fetch=False)
    engine.expand()
    for name in ("rising", "rising", "reference"):              # any call, also one that changes nothing
        engine.set_data_term(name)
        with pytest.raises(mh.MultiHError) as ei:
            engine.expand()
        assert ei.value.code == -4 and "stale" in str(ei.value)
        engine.data_cost(fetch=False)
        engine.expand()
    for bad in (2, -1, 7):
        assert engine.lib.mh_set_data_term(engine._h, bad) == -2
    assert engine.lib.mh_set_data_term(None, 1) == -2
    with pytest.raises(ValueError):
        engine.set_data_term("falling")
    engine.expand()                                              # a refused value changed nothing
    # sticky: mh_set_correspondences does not reset it
    engine.set_data_term("rising")
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_models(sc.H_true)
    assert np.array_equal(engine.data_cost(), T.cost_table(sc.src, sc.dst, sc.H_true, 0.5, THR2, T.RISING))


@pytest.mark.parametrize("ctx", [1, 16])
@pytest.mark.parametrize("n,k,seed", [(2000, 5, 3), (300, 3, 2)])
def test_labeling_step_under_the_rising_term(engine, synth, n, k, seed, ctx):
    """mh_labeling_step cold, then warm, as tests/test_gpu_parity.py::test_labeling_step_and_loop runs it under the default
    term: labels, energy and cycles equal, the HAF refits held to that test's assertion; with the alpha-moves one after the
    other (key 37 = 1) and sixteen at a time."""
    sc = synth.make_scene(n, k, seed=seed)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_epipolar(sc.F, sc.e2)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    engine.set_tuning(37, ctx)
    engine.set_data_term("rising")
    H = sc.H_true * (1.0 + np.random.default_rng(seed).normal(0, 1e-4, size=sc.H_true.shape))
    engine.set_models(H)
    lab = np.full(sc.n, -1, dtype=np.int32)
    lab_ref, H_ref = lab.copy(), H.copy()
    lab_default = None
    for it in range(4):
        warm = it > 0
        lab, energy, cycles = engine.labeling_step(warm, lab)
        lab_ref, H_ref, e_ref, cyc_ref = T.labeling_step_twin(sc.src, sc.dst, sc.aff, H_ref, 0.5, THR2, sc.hit_rowptr, sc.hit_col,
                                                              warm, sc.F, sc.e2, lab_ref, T.RISING)
        if it == 0:
            lab_default = T.labeling_step_twin(sc.src, sc.dst, sc.aff, H, 0.5, THR2, sc.hit_rowptr, sc.hit_col, False, sc.F, sc.e2,
                                               lab_ref, T.REFERENCE)
        if it == 0:
            assert lab_default[2] != e_ref, "the two terms give different energies on this scene"
        assert energy == e_ref and cycles == cyc_ref, f"iteration {it}"
        assert np.array_equal(lab, lab_ref), f"iteration {it}"
        Hg = engine.get_models()
        scale = np.max(np.abs(H_ref), axis=1, keepdims=True)
        assert np.max(np.abs(Hg - H_ref) / scale) <= 1e-6
        assert np.array_equal(Hg.view(np.uint64), H_ref.view(np.uint64)), f"iteration {it}"


def _host(mh):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_data_term.argtypes = [C.c_int]
    host.mhh_set_data_term.restype = None
    return host


@pytest.mark.parametrize("n,planes,seed,duplicates,strays", [(300, 3, 2, 2, 1), (2000, 5, 11, 2, 1)])
def test_process_loop_under_the_rising_term_equals_the_twin(mh, engine_lib, synth, oracle, n, planes, seed, duplicates, strays):
    """The whole merge <-> label loop through the host class, from given initial models with the post-filter off, as
    tests/test_gpu_alternation.py::test_process_loop_equals_the_oracle_alternation[post_filter False] with the same assertions;
    then once more without the hook: it does not stick, and the default is the oracle's loop."""
    sc = synth.make_scene(n, planes, seed=seed, with_neighbours=False)
    H0 = alt._initial_models(sc, seed, duplicates, strays)
    rowptr, col = alt._knn_hits(sc, 16)
    host = _host(mh)
    lab, H, it, en = T.loop_twin(sc.src, sc.dst, sc.aff, H0, sc.F, sc.e2, alt.LAM, alt.THR, rowptr, col, seed, T.RISING)
    want = {"labels": lab, "H": H, "iterations": it, "energy": en}
    host.mhh_set_data_term(1)
    try:
        got = alt._run_process(mh, sc, seed, H0=H0, post_filter=False)
    finally:
        host.mhh_set_data_term(-1)
    alt._assert_same_result(got, want)
    assert got[0] >= 2 and want["iterations"] >= 1
    lab_o, H_o, it_o, en_o, _ = oracle.cluster_merging_and_labeling(sc.src, sc.dst, sc.aff, H0, sc.F, sc.e2, alt.LAM, alt.THR, rowptr,
                                                                    col, seed)
    again = alt._run_process(mh, sc, seed, H0=H0, post_filter=False)
    alt._assert_same_result(again, {"labels": lab_o, "H": H_o, "iterations": it_o, "energy": en_o})
    assert en_o != en, "the two terms give different energies on this scene"
    host.mhh_set_data_term(2)                                   # an unknown term: Process() fails, with the engine's message
    try:
        assert alt._run_process(mh, sc, seed, H0=H0, post_filter=False)[0] == -1
    finally:
        host.mhh_set_data_term(-1)


def test_harness_data_term_flag(mh, tmp_path):
    sc = mh.synth.make_scene(2000, 3, seed=37, with_neighbours=False)
    corr = tmp_path / "in.txt"
    np.savetxt(corr, np.concatenate([sc.src, sc.dst], axis=1), fmt="%.17g")
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    outs = {}
    for name, extra in (("plain", []), ("reference", ["--data-term", "reference"]), ("rising", ["--data-term", "rising"])):
        out = tmp_path / f"{name}.out"
        r = subprocess.run([harness, str(corr), str(out), "--points", *extra], capture_output=True, text=True, timeout=40)
        assert r.returncode == 0, name + r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = open(out).read()
    assert outs["reference"] == outs["plain"]
    assert np.loadtxt(tmp_path / "rising.out", ndmin=2).shape[1] == 5
    r = subprocess.run([harness, str(corr), str(tmp_path / "bad.out"), "--points", "--data-term", "falling"], capture_output=True,
                       text=True, timeout=40)
    assert r.returncode == 2 and "--data-term" in r.stderr
