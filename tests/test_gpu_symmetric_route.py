"""GPU tests of the symmetric route (mh_set_residual_scope(MH_RESIDUAL_SCOPE_ROUTE) under MH_RESIDUAL_SYMMETRIC,
include/multih_hip.h; MultiH::SetResidual) against the numpy twin of tests/symmetric_route_numpy.py and the oracle's symmetric
residual.  Every comparison is exact: integers equal, doubles bit for bit.

The cost tables: k_data_cost<., true> and k_cost_matrix<16, ., true> at the sizes where the kernels take another path — the
256-thread edge, the int4 store and its tail, the 1 024-point tile and more than one point slice (atomics on the counts), the
16-model block — on models that make d2 = 0, a non-finite d2 through H and through adj(H), a singular H, d2 within a few ulp
of T on either side, and far pairs; whatever mh_set_tuning keys 15 and 23 say."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import data_term_numpy as T
import symmetric_route_numpy as S
import test_gpu_alternation as alt

pytestmark = pytest.mark.gpu
THR, LOCALITY = 2.2, 0.005
THR2 = THR * THR
NS = (1, 3, 255, 1024, 1025, 4099)
MS = (1, 15, 16, 17, 33)
SCENES = [(300, 3, 2, 1.0), (2000, 5, 3, 1.0), (2000, 5, 3, 0.5)]          # n, planes, seed, thr_hom: tests/test_symmetric_route_cpu.py


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _near_half_T_offsets():
    """Offsets dx with 2 * fl(dx * dx) within a few ulp of T = thr^2 81/16, on both sides of it."""
    Tt = THR2 * 81.0 / 16.0
    dx = [np.sqrt(Tt / 2.0)]
    for _ in range(3):
        dx.insert(0, np.nextafter(dx[0], 0.0))
        dx.append(np.nextafter(dx[-1], np.inf))
    return np.array(dx), Tt


def scene_models(sc, seed):
    return sc.H_true * (1.0 + np.random.default_rng(seed).normal(0, 1e-4, size=sc.H_true.shape))


@pytest.fixture(scope="module")
def pool(synth, oracle):
    """4 099 points and 33 models, and both errors of every pair (the oracle's, bit-equal to the engine's), once."""
    sc = synth.make_scene(4099, 3, seed=5, with_neighbours=False)
    src, dst = sc.src.copy(), sc.dst.copy()
    dx, Tt = _near_half_T_offsets()
    # against the identity (model 0): src = (0, 0), dst = (dx, 0) -> forward fl(dx * dx), backward the same: d2 = 2 fl(dx * dx)
    # exactly.  Model 1 = [1 0 0; 0 1 0; -0.5 0 1]: s = 0 at src x = 2 (forward inf / NaN); adj's third row is (0.5, 0, 1):
    # s = 0 under adj(H) at dst x = -2.  Model 2 adds 0 / 0 forward at (2, 1).  Model 3 has rank 1: adj(H) = 0 exactly, so the
    # backward term is 0 / 0 for every pair.
    special = [((0.0, 0.0), (dx[3], 0.0)), ((2.0, 1.0), (5.0, 7.0)), ((5.0, 7.0), (-2.0, 1.0))]
    special += [((0.0, 0.0), (v, 0.0)) for v in dx] + [((0.0, 0.0), (0.0, 0.0)), ((2.0, 1.0), (2.0, 1.0))]
    for at in (0, 1018, 4099 - len(special)):                   # the first points (n = 1, 3), across the tile edge, the tail
        for j, (s, d) in enumerate(special):
            src[at + j], dst[at + j] = s, d
    rng = np.random.default_rng(5)
    H = [np.eye(3).reshape(9), np.array([1, 0, 0, 0, 1, 0, -0.5, 0, 1.0]), np.array([1, 0, -2.0, 0, 1, 0, -0.5, 0, 1.0]),
         np.array([1, 1, 1, 2, 2, 2, 1, 1, 1.0])]
    H += list(sc.H_true)
    while len(H) < 33:
        if len(H) % 2:
            H.append(sc.H_true[len(H) % 3] * (1.0 + rng.normal(0, 1e-3, size=9)))       # near a plane: many pairs inside T
        else:
            H.append((np.eye(3) + rng.normal(0, 0.05, size=(3, 3))).reshape(9))          # far from everything
    H = np.ascontiguousarray(np.array(H))
    with np.errstate(all="ignore"):
        d2f = oracle.residual_matrix(src, dst, H)
        d2s = oracle.residual_matrix_sym(src, dst, H)
        back1 = oracle.residual_matrix(dst, src, np.array([[1, 0, 0, 0, 1, 0, 0.5, 0, 1.0]]))[0]      # adj(model 1), exact
    ulp = np.spacing(Tt)
    row = d2s[0]
    assert ((row < Tt) & (Tt - row <= 8 * ulp)).any() and ((row >= Tt) & (row - Tt <= 8 * ulp)).any(), "near-miss pairs on both sides of T"
    assert np.array_equal(_bits(row[3:3 + len(dx)]), _bits(2.0 * (dx * dx)))
    assert (row == 0.0).any()
    assert (~np.isfinite(d2f[1])).any(), "s = 0 under H"
    assert (np.isfinite(d2f[1]) & ~np.isfinite(back1)).any() and (np.isfinite(d2f[1]) & ~np.isfinite(d2s[1])).any(), "s = 0 under adj(H) alone"
    assert np.isnan(d2s[2]).any()
    assert np.isnan(d2s[3]).all() and np.isfinite(d2f[3]).any(), "the singular model: every symmetric error is NaN"
    assert (d2s[4:] < Tt).mean() > 0.02 and (d2s[4:] > 100 * Tt).mean() > 0.2
    assert ((d2f < Tt) & ~(d2s < Tt)).sum() > 100, "pairs that the two errors cost differently"
    with np.errstate(all="ignore"):
        cnt_sym = {n: oracle.score_sym(src[:n], dst[:n], H, THR2) for n in NS}
        cnt_fwd = {n: oracle.score(src[:n], dst[:n], H, THR2) for n in NS}
    return dict(src=src, dst=dst, H=H, d2f=d2f, d2s=d2s, cnt_sym=cnt_sym, cnt_fwd=cnt_fwd)


def _route(engine, on=True):
    engine.set_residual_mode(bool(on))
    engine.set_residual_scope("route" if on else "score")


# ---- 1. tables -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key23", ["default", 0])
@pytest.mark.parametrize("key15", [1, 0])
@pytest.mark.parametrize("term", ["reference", "rising"])
def test_tables_equal_the_twin_and_the_scope_leaks_nothing(engine, oracle, pool, term, key15, key23):
    src, dst, H = pool["src"], pool["dst"], pool["H"]
    lam = 0.5
    engine.set_params(2.6, THR, LOCALITY, lam, 20)
    engine.set_tuning(15, key15)
    if key23 != "default":
        engine.set_tuning(23, key23)
    engine.set_data_term(term)
    t = T.RISING if term == "rising" else T.REFERENCE
    want = T.term_of_d2(pool["d2s"], lam, THR2, t)              # [model, point]
    forward = T.term_of_d2(pool["d2f"], lam, THR2, t)
    if t == T.REFERENCE:
        assert np.array_equal(forward, oracle.data_cost(src, dst, H, lam, THR2)[:, 1:].T)
    assert np.array_equal(want, S.cost_matrix(src, dst, H, lam, THR2, t))
    B = T.outlier_cost(lam, THR2)
    assert (want[3] == 2 * B).all(), "a singular H costs 2B everywhere"
    for n in NS:
        engine.set_correspondences(src[:n], dst[:n])
        for m in MS:
            where = (term, key15, key23, n, m)
            engine.set_models(H[:m])
            _route(engine, True)
            Cm, cnt = engine.cost_matrix()
            cost = engine.data_cost()
            assert np.array_equal(Cm, want[:m, :n]), where
            assert np.array_equal(cost[:, 1:], Cm.T) and np.all(cost[:, 0] == B), where
            assert np.array_equal(cnt, pool["cnt_sym"][n][:m]), where
            # ... and back: the forward launches again
            engine.set_residual_scope("score")
            Cm_back, cnt_back = engine.cost_matrix()
            cost_back = engine.data_cost()
            engine.set_residual_mode(False)
            assert np.array_equal(Cm_back, forward[:m, :n]) and np.array_equal(cost_back[:, 1:], forward[:m, :n].T), where
            assert np.all(cost_back[:, 0] == B) and np.array_equal(cnt_back, pool["cnt_fwd"][n][:m]), where
    assert not np.array_equal(want, forward)


# ---- 2. scope off is today's behaviour -------------------------------------------------------------------------------------

def test_the_mode_alone_changes_nothing_behind_the_selection(engine, oracle, pool):
    n, m = 1025, 17
    src, dst, H = pool["src"][:n], pool["dst"][:n], pool["H"][:m]
    engine.set_params(2.6, THR, LOCALITY, 0.5, 20)
    engine.set_correspondences(src, dst)
    engine.set_models(H)
    with np.errstate(all="ignore"):
        cost_ref = oracle.data_cost(src, dst, H, 0.5, THR2)
        mo_ref, me_ref = oracle.inlier_moments(src, dst, H, THR2)
    cnt_ref = pool["cnt_fwd"][n][:m]
    lab0 = np.arange(n, dtype=np.int32) % 7 - 3
    idx = 5                                                      # a model near a plane
    lab_ref = np.where(pool["d2f"][idx, :n] < THR2, 99, lab0).astype(np.int32)

    def outputs():
        Cm, cnt = engine.cost_matrix()
        mo, me = engine.inlier_moments(THR2)
        return engine.data_cost(), Cm, cnt, mo, me, engine.inliers_of_model(idx, THR2, 99, lab0), engine.inliers_of_homography(H[idx], THR2, 99, lab0)

    engine.set_residual_mode(True)                               # scope "score", the default
    cost, Cm, cnt, mo, me, lab, lab_h = outputs()
    ok = ~np.isnan(mo_ref).any(axis=1)
    assert np.array_equal(cost, cost_ref) and np.array_equal(Cm, cost_ref[:, 1:].T) and np.array_equal(cnt, cnt_ref)
    assert np.array_equal(_bits(mo[ok]), _bits(mo_ref[ok])) and np.array_equal(mo[:, 0], mo_ref[:, 0])
    assert np.array_equal(_bits(me[ok]), _bits(me_ref[ok]))
    assert np.array_equal(lab, lab_ref) and np.array_equal(lab_h, lab_ref)
    engine.set_residual_scope("route")
    cost2, Cm2, cnt2, mo2, me2, lab2, lab_h2 = outputs()
    assert not np.array_equal(cost2, cost_ref) and not np.array_equal(Cm2, Cm) and not np.array_equal(cnt2, cnt_ref)
    assert not np.array_equal(mo2[:, 0], mo_ref[:, 0])
    assert not np.array_equal(lab2, lab_ref) and np.array_equal(lab_h2, lab2)


# ---- 3. moments ------------------------------------------------------------------------------------------------------------

def _moment_cases(mh, pool):
    for n, k, seed in ((300, 3, 2), (2000, 5, 3)):
        sc = mh.synth.make_scene(n, k, seed=seed, with_neighbours=False)
        yield f"scene {n}/{k}", sc.src, sc.dst, scene_models(sc, seed)
    for n in (2047, 2048, 2049):                                 # the kernel's 8 x 256 stride
        yield f"pool {n}", pool["src"][:n], pool["dst"][:n], pool["H"][[0, 4, 5, 7]]


def test_moments_are_the_forward_moments_of_the_symmetric_inliers(mh, engine, oracle, pool):
    """The sums read only first-image coordinates of the inliers, at their indices, and a symmetric inlier is a forward
    inlier: send every other point's second-image coordinates far away and the FORWARD moments are the symmetric ones."""
    thr2 = 1.0
    for name, src, dst, H in _moment_cases(mh, pool):
        engine.set_correspondences(src, dst)
        engine.set_models(H)
        _route(engine, True)
        mo, me = engine.inlier_moments(thr2)
        _route(engine, False)
        mo_f, _ = engine.inlier_moments(thr2)
        with np.errstate(all="ignore"):
            inl = oracle.residual_matrix_sym(src, dst, H) < thr2
            inl_f = oracle.residual_matrix(src, dst, H) < thr2
        assert np.array_equal(mo[:, 0], inl.sum(axis=1)) and np.array_equal(mo_f[:, 0], inl_f.sum(axis=1)), name
        assert (inl.sum(axis=1) >= 3).all() and (inl_f & ~inl).any(), name
        for m in range(H.shape[0]):
            far = dst.copy()
            far[~inl[m]] = (1.0e6, -1.0e6)
            engine.set_correspondences(src, far)
            engine.set_models(H[m:m + 1])
            mo_e, me_e = engine.inlier_moments(thr2)
            mo_o, me_o = oracle.inlier_moments(src, far, H[m:m + 1], thr2)
            assert mo_o[0, 0] == inl[m].sum(), (name, m)
            assert np.array_equal(_bits(mo[m]), _bits(mo_e[0])) and np.array_equal(_bits(mo[m]), _bits(mo_o[0])), (name, m)
            assert _bits(me[m]) == _bits(me_e[0]) and _bits(me[m]) == _bits(me_o[0]), (name, m)


# ---- 4. single-model labelling -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 2000])
def test_inliers_of_model_and_of_homography(engine, pool, n):
    src, dst, H = pool["src"][:n], pool["dst"][:n], pool["H"][:8]
    engine.set_correspondences(src, dst)
    engine.set_models(H)
    _route(engine, True)
    lab0 = (np.arange(n, dtype=np.int32) * 7) % 11 - 5           # a pre-filled array: the other entries stay
    seen_nan = False
    for idx in range(H.shape[0]):
        d2 = pool["d2s"][idx, :n]
        want = np.where(d2 < THR2, 40 + idx, lab0).astype(np.int32)          # strictly; a NaN row stays
        seen_nan |= bool(np.isnan(d2).any())
        assert np.array_equal(engine.inliers_of_model(idx, THR2, 40 + idx, lab0), want), idx
        assert np.array_equal(engine.inliers_of_homography(H[idx], THR2, 40 + idx, lab0), want), idx
        if n == 2000 and idx >= 4 and idx % 2:
            assert (want != lab0).any() and (want == lab0).any()
            assert not np.array_equal(want, np.where(pool["d2f"][idx, :n] < THR2, 40 + idx, lab0)), idx
    assert seen_nan
    assert engine.get_models().shape[0] == 8                     # _of_homography leaves the model set alone


# ---- 5. labeling -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ctx", [1, 16])
@pytest.mark.parametrize("n,k,seed,thr", SCENES)
def test_labeling_step_under_the_symmetric_route(mh, engine, n, k, seed, thr, ctx):
    """mh_labeling_step cold, then three warm steps, as tests/test_gpu_data_term.py runs it under the rising term: labels,
    energy and cycles equal the twin's, the models bit-equal to the HAF refits of the twin's labels."""
    sc = mh.synth.make_scene(n, k, seed=seed)
    thr2 = thr * thr
    engine.set_params(2.6, thr, LOCALITY, 0.5, 20)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_epipolar(sc.F, sc.e2)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    engine.set_tuning(37, ctx)
    _route(engine, True)
    H = scene_models(sc, seed)
    engine.set_models(H)
    lab = np.full(sc.n, -1, dtype=np.int32)
    lab_ref, H_ref = lab.copy(), H.copy()
    for it in range(4):
        warm = it > 0
        lab, energy, cycles = engine.labeling_step(warm, lab)
        if it == 0:
            e_fwd = T.labeling_step_twin(sc.src, sc.dst, sc.aff, H, 0.5, thr2, sc.hit_rowptr, sc.hit_col, False, sc.F, sc.e2, lab_ref,
                                         T.REFERENCE)[2]
        lab_ref, H_ref, e_ref, cyc_ref = S.labeling_step_twin(sc.src, sc.dst, sc.aff, H_ref, 0.5, thr2, sc.hit_rowptr, sc.hit_col, warm,
                                                              sc.F, sc.e2, lab_ref)
        if it == 0:
            assert e_fwd != e_ref and energy != e_fwd, "the two errors give different energies on this scene"
        assert energy == e_ref and cycles == cyc_ref, f"iteration {it}"
        assert np.array_equal(lab, lab_ref), f"iteration {it}"
        assert np.array_equal(_bits(engine.get_models()), _bits(H_ref)), f"iteration {it}"


# ---- 6. state --------------------------------------------------------------------------------------------------------------

def test_scope_state(mh, engine, synth):
    sc = synth.make_scene(300, 3, seed=2)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_epipolar(sc.F, sc.e2)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    engine.set_models(sc.H_true)
    engine.data_cost(fetch=False)
    engine.expand()

    def stale():
        with pytest.raises(mh.MultiHError) as ei:
            engine.expand()
        assert ei.value.code == -4 and "stale" in str(ei.value)
        engine.data_cost(fetch=False)
        engine.expand()

    for name in ("route", "route", "score", "score"):            # any call, also one that changes nothing
        engine.set_residual_scope(name)
        stale()
    # the mode marks the cost stale under "route" and does not under "score"
    engine.set_residual_mode(True)
    engine.expand()
    engine.set_residual_mode(False)
    engine.expand()
    engine.set_residual_scope("route")
    engine.data_cost(fetch=False)
    for symmetric in (True, True, False):
        engine.set_residual_mode(symmetric)
        stale()
    # bad values and a null engine: MH_ERR_INVALID, nothing changed
    for bad in (2, -1, 7):
        assert engine.lib.mh_set_residual_scope(engine._h, bad) == -2
    assert engine.lib.mh_set_residual_scope(None, 1) == -2
    with pytest.raises(ValueError):
        engine.set_residual_scope("everything")
    engine.expand()                                              # a refused value left the cost fresh ...
    engine.set_residual_mode(True)
    stale()                                                      # ... and the scope "route"
    # sticky: mh_set_correspondences resets neither
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_models(sc.H_true)
    assert np.array_equal(engine.data_cost(), S.cost_table(sc.src, sc.dst, sc.H_true, 0.5, THR2))
    assert not np.array_equal(engine.data_cost(), T.cost_table(sc.src, sc.dst, sc.H_true, 0.5, THR2, T.REFERENCE))
    # the MSAC scores stay forward-only
    with pytest.raises(mh.MultiHError) as ei:
        engine.score_msac(THR2)
    assert ei.value.code == -2 and "forward residual only" in str(ei.value)
    with pytest.raises(mh.MultiHError) as ei:
        engine.select_greedy_msac(THR2, 20, 4)
    assert ei.value.code == -2 and "forward residual only" in str(ei.value)


# ---- 7. the class and the harness ------------------------------------------------------------------------------------------

def _host(mh):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_residual.argtypes = [C.c_int]
    host.mhh_set_residual.restype = None
    host.mhh_set_epipolar_free.argtypes = [C.c_int]
    host.mhh_set_epipolar_free.restype = None
    host.mhh_set_tail_score.argtypes = [C.c_int]
    host.mhh_set_tail_score.restype = None
    return host


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[2]), _bits(b[2])) and a[3] == b[3] and a[4] == b[4]


@pytest.mark.parametrize("epipolar_free", [False, True])
@pytest.mark.parametrize("n,k,seed", [(300, 3, 2), (2000, 5, 3)])
def test_process_under_the_symmetric_route(mh, engine_lib, n, k, seed, epipolar_free):
    sc = mh.synth.make_scene(n, k, seed=seed, with_neighbours=False)
    host = _host(mh)
    host.mhh_set_epipolar_free(1 if epipolar_free else 0)
    try:
        before = alt._run_process(mh, sc, seed, hypotheses=2000)           # forward, the setter untouched
        host.mhh_set_residual(1)
        first = alt._run_process(mh, sc, seed, hypotheses=2000)
        second = alt._run_process(mh, sc, seed, hypotheses=2000)
        host.mhh_set_residual(-1)
        after = alt._run_process(mh, sc, seed, hypotheses=2000)            # the pooled engine comes back in symmetric mode: the class sets both ways
        host.mhh_set_residual(0)
        after0 = alt._run_process(mh, sc, seed, hypotheses=2000)
        host.mhh_set_residual(7)
        assert alt._run_process(mh, sc, seed, hypotheses=2000)[0] == -1    # an unknown value: Process() fails
        host.mhh_set_residual(1)
        host.mhh_set_tail_score(1)
        assert alt._run_process(mh, sc, seed, hypotheses=2000)[0] == -1    # the MSAC tail is forward-only
    finally:
        host.mhh_set_residual(-1)
        host.mhh_set_tail_score(-1)
        host.mhh_set_epipolar_free(0)
    kk, labels, H, _, _ = first
    print(f"{n}/{k} seed {seed} epipolar_free {epipolar_free}: forward {before[0]} models, symmetric {kk} models")
    assert before[0] >= 0 and kk >= 0
    assert np.isfinite(H).all()
    assert labels.min() >= -1 and labels.max() < max(kk, 1)
    assert _same(first, second)
    assert _same(after, before) and _same(after0, before)


def test_harness_residual_flag(mh, tmp_path):
    sc = mh.synth.make_scene(2000, 3, seed=37, with_neighbours=False)
    corr = tmp_path / "in.txt"
    np.savetxt(corr, np.concatenate([sc.src, sc.dst], axis=1), fmt="%.17g")
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    outs = {}
    for name, extra in (("plain", []), ("forward", ["--residual", "forward"]), ("symmetric", ["--residual", "symmetric"])):
        out = tmp_path / f"{name}.out"
        r = subprocess.run([harness, str(corr), str(out), "--points", *extra], capture_output=True, text=True, timeout=40)
        assert r.returncode == 0, name + r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = open(out).read()
    assert outs["forward"] == outs["plain"]
    assert np.loadtxt(tmp_path / "symmetric.out", ndmin=2).shape[1] == 5
    r = subprocess.run([harness, str(corr), str(tmp_path / "bad.out"), "--points", "--residual", "bogus"], capture_output=True,
                       text=True, timeout=40)
    assert r.returncode == 2 and "--residual: forward or symmetric" in r.stderr
    r = subprocess.run([harness, str(corr), str(tmp_path / "bad.out"), "--points", "--residual", "symmetric", "--tail-score", "msac"],
                       capture_output=True, text=True, timeout=40)
    assert r.returncode != 0 and "do not combine with RESIDUAL_SYMMETRIC" in r.stderr
