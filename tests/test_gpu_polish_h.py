"""mh_polish_homographies (csrc/polish_h.hip, k_polish_h), the polished degenerate tail (MultiH::SetTailPolish) and the final
polish of Process() (MultiH::SetModelPolish) on the GPU, against the numpy twin of the rule in include/multih_hip.h
(tests/polish_h_numpy.py): H_out and cost as uint64 bits, info exactly.  The seeds of the chosen cases were found on the CPU
with the twin; every such case asserts that it is what it was chosen for."""
import ctypes as C
import os

import numpy as np
import pytest

import polish_h_numpy as P
import refit_h_numpy as T
import test_gpu_alternation as alt

pytestmark = pytest.mark.gpu
THR2 = 2.2 * 2.2
IDENT = np.eye(3).reshape(9)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _held_to_the_twin(engine, src, dst, labels, H_in, iterations, traces=None):
    """One call against the twin; returns the twin's (H_out, cost, info)."""
    H, cost, info = P.polish(src, dst, labels, H_in, iterations, traces)
    gH, gcost, ginfo = engine.polish_homographies(labels, H_in, iterations)
    assert np.array_equal(ginfo, info), (iterations, ginfo.tolist(), info.tolist())
    assert np.array_equal(_bits(gcost), _bits(cost)), (iterations, gcost, cost)
    assert np.array_equal(_bits(gH), _bits(H)), (iterations, gH, H)
    return H, cost, info


def _off_by_a_pixel(H_true, rng):
    H0 = H_true / H_true[8]
    H0[2] += rng.normal(0, 1.0)
    H0[5] += rng.normal(0, 1.0)
    return H0


@pytest.mark.parametrize("n", [4, 5, 255, 256, 257, 513, 2000])
def test_stride_and_membership_edges(engine, n):
    """The member counts at which the 256-thread sums change shape: fewer members than threads, exactly one per thread, one
    thread with two, two full trips and one over, many trips; 30 % of the points carry another label (1: polished too, from the
    identity) or none (-1), interleaved, so the members of a thread are not consecutive trips."""
    rng = np.random.default_rng(n)
    others = max(int(0.3 * n), 1)
    src, dst, H_true, good = T.plane_scene(rng, n, 0.5, outliers=others)
    labels = np.where(good, 0, np.where(rng.random(n + others) < 0.5, 1, -1)).astype(np.int32)
    H_in = np.stack([_off_by_a_pixel(H_true, rng), IDENT])
    engine.set_correspondences(src, dst)
    seen = [_held_to_the_twin(engine, src, dst, labels, H_in, it) for it in (0, 1, 10, 32)]
    assert all(s[2][0, 0] == n and s[2][0, 3] == 0 for s in seen)
    assert np.array_equal(_bits(seen[0][0][0]), _bits(H_in[0])) and tuple(seen[0][2][0]) == (n, 0, 0, 0)
    if n >= 255:
        assert seen[2][2][0, 2] >= 2 and seen[2][1][0, 1] < seen[2][1][0, 0]            # (not vacuous: steps were taken and kept)
        assert seen[2][2][0, 1] < 10                                                    # ... and the loop ended on its own


@pytest.mark.parametrize("m", [1, 2, 17])
def test_membership_edges(engine, m):
    """m models; the last label has no member and — for m > 2 — the one before it three; labels -1, m, m + 5 and a large value
    belong to nobody; labels 0 and 1 (m = 17) alternate point by point."""
    rng = np.random.default_rng(40 + m)
    n = 1200
    src, dst, H_true, _ = T.plane_scene(rng, n, 0.5)
    full = max(m - 2, 1) if m > 1 else 1
    labels = rng.integers(0, full, size=n).astype(np.int32)
    if m == 17:
        labels[:400] = np.arange(400) % 2
    stray = rng.choice(n, 90, replace=False)
    labels[stray[:30]], labels[stray[30:60]], labels[stray[60:80]], labels[stray[80:]] = -1, m, m + 5, 2 ** 30
    if m > 2:
        labels[rng.choice(np.flatnonzero(labels == 0), 3, replace=False)] = m - 2
    H_in = np.stack([_off_by_a_pixel(H_true, rng) * s for s in rng.uniform(0.5, 3.0, size=m)])
    engine.set_correspondences(src, dst)
    for it in (0, 3, 10):
        H, cost, info = _held_to_the_twin(engine, src, dst, labels, H_in, it)
        assert info[:, 0].sum() == int(((labels >= 0) & (labels < m)).sum())
        if m > 1:
            assert tuple(info[m - 1]) == (0, 0, 0, 1) and np.array_equal(_bits(H[m - 1]), _bits(H_in[m - 1]))
        if m > 2:
            assert tuple(info[m - 2]) == (3, 0, 0, 1) and np.array_equal(_bits(H[m - 2]), _bits(H_in[m - 2]))
        assert np.all(info[:full, 3] == 0) and (it == 0 or np.all(info[:full, 2] >= 1))


def test_degenerate_inputs(engine):
    rng = np.random.default_rng(53)
    src, dst, H_true, _ = T.plane_scene(rng, 300, 0.5)
    labels = (np.arange(300) % 3).astype(np.int32)
    # H_in[8] = 0 and a NaN entry: status 2, the bits of H_in; the third model is polished as ever
    H_zero, H_nan = H_true.copy(), H_true.copy()
    H_zero[8], H_nan[1] = 0.0, np.nan
    H_in = np.stack([H_zero, H_nan, H_true])
    engine.set_correspondences(src, dst)
    for it in (0, 10):
        H, cost, info = _held_to_the_twin(engine, src, dst, labels, H_in, it)
        assert info[:, 3].tolist() == [2, 2, 0] and info[:, 0].tolist() == [100, 100, 100]
        assert np.array_equal(_bits(H[:2]), _bits(H_in[:2])) and np.all(cost[:2] == 0.0)
    # a member exactly on the model's line at infinity: x6 * 512 + 1 == 0, the ww = 0 branch
    H_inf = np.array([1.0, 0, 0, 0, 1.0, 0, -1.0 / 512.0, 0, 1.0])
    src2, dst2 = src.copy(), dst.copy()
    src2[:, 0] = rng.uniform(0, 400, size=300)
    q = np.concatenate([src2, np.ones((300, 1))], axis=1) @ H_inf.reshape(3, 3).T
    dst2 = q[:, :2] / q[:, 2:3] + rng.normal(0, 0.5, size=(300, 2))
    src2[7] = [512.0, 130.0]
    dst2[7] = [3.0, -2.0]
    assert P.residuals(src2, dst2, np.array([7]), H_inf[:8])[0][0] == 0.0
    engine.set_correspondences(src2, dst2)
    one = np.zeros(300, np.int32)
    for it in (0, 1, 10):
        H, cost, info = _held_to_the_twin(engine, src2, dst2, one, H_inf, it)
    assert cost[0, 0] >= 13.0                                                # (the member's residual is -(u, v): 9 + 4)
    # collinear members: A is singular and the cut drops eigenvalues; whatever the rule gives
    src3 = np.stack([25.0 * np.arange(40), 3.0 + 0.5 * 25.0 * np.arange(40)], axis=1)
    q = np.concatenate([src3, np.ones((40, 1))], axis=1) @ H_true.reshape(3, 3).T
    dst3 = q[:, :2] / q[:, 2:3] + rng.normal(0, 0.5, size=(40, 2))
    engine.set_correspondences(src3, dst3)
    for it in (1, 10, 32):
        traces = []
        _held_to_the_twin(engine, src3, dst3, np.zeros(40, np.int32), _off_by_a_pixel(H_true, rng), it, traces)
    assert sum(t[4] for t in traces[0]) >= 1, "the scene should make the cut drop an eigenvalue"


@pytest.mark.parametrize("seed,iterations", [(500, 32), (607, 32)])
def test_a_far_start_with_rejected_steps(engine, seed, iterations):
    """A 4-point hypothesis of 300 noisy points, far enough off that steps are rejected in the middle of the run (an accepted
    step follows a rejected one), the lambda == 0 branch is taken and the cut drops an eigenvalue."""
    rng = np.random.default_rng(seed)
    src, dst, _, _ = T.plane_scene(rng, 300, 0.5)
    H0 = T.fit(src, dst, np.sort(rng.choice(300, 4, replace=False)))
    engine.set_correspondences(src, dst)
    traces = []
    H, cost, info = _held_to_the_twin(engine, src, dst, np.zeros(300, np.int32), H0, 32, traces)
    tr = traces[0]
    accepted = [t[2] for t in tr]
    assert info[0, 1] == iterations and len(tr) == iterations
    assert any(not a and any(accepted[i + 1:]) for i, a in enumerate(accepted)), "a rejected step in the middle"
    assert any(t[3] for t in tr) and sum(t[4] for t in tr) >= 1
    assert cost[0, 1] < cost[0, 0]
    for it in (1, 2, 5):
        _held_to_the_twin(engine, src, dst, np.zeros(300, np.int32), H0, it)


def test_engine_state_is_untouched(engine):
    rng = np.random.default_rng(2)
    src, dst, H_true, good = T.plane_scene(rng, 1050, 1.0, outliers=450)
    labels = np.where(good, 0, -1).astype(np.int32)
    engine.set_correspondences(src, dst)

    def run(with_polish):
        engine.propose_dlt4(77, 0, 600)
        counts = engine.score(THR2)
        if with_polish:
            engine.polish_homographies(labels, H_true, 10)
        best = engine.select_best()
        if with_polish:
            engine.polish_homographies(np.arange(1500) % 5, np.tile(H_true, (5, 1)), 2)
        return engine.model_count, engine.get_models(), counts, best, engine.score(THR2)

    plain, mixed = run(False), run(True)
    assert plain[0] == mixed[0] == 600 and plain[3] == mixed[3] and plain[3][1] == int(plain[2].max())
    assert np.array_equal(_bits(plain[1]), _bits(mixed[1]))
    assert np.array_equal(plain[2], mixed[2]) and np.array_equal(plain[4], mixed[4]) and np.array_equal(plain[2], plain[4])


def test_error_codes(mh, engine):
    lib, h = engine.lib, engine._h
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    H, out, lab = np.tile(IDENT, (2, 1)), np.empty((2, 9)), np.zeros(50, np.int32)
    Hp, op, lp = H.ctypes.data_as(dp), out.ctypes.data_as(dp), lab.ctypes.data_as(ip)
    call = lambda *a: lib.mh_polish_homographies(*a, None, None)
    assert call(h, lp, Hp, 1, 1, op) == -4                                   # MH_ERR_NOT_SET: no correspondences yet
    rng = np.random.default_rng(3)
    src, dst, _, _ = T.plane_scene(rng, 50, 0.5)
    engine.set_correspondences(src, dst)
    assert call(h, lp, Hp, 1, 1, op) == 0 and call(h, lp, Hp, 2, 0, op) == 0 and call(h, lp, Hp, 2, 32, op) == 0
    assert call(None, lp, Hp, 1, 1, op) == -2
    assert call(h, None, Hp, 1, 1, op) == -2
    assert call(h, lp, None, 1, 1, op) == -2
    assert call(h, lp, Hp, 1, 1, None) == -2
    assert call(h, lp, Hp, 0, 1, op) == -2 and call(h, lp, Hp, -1, 1, op) == -2
    assert call(h, lp, Hp, 65537, 1, op) == -2                               # (refused before anything of that size is read)
    assert call(h, lp, Hp, 1, -1, op) == -2 and call(h, lp, Hp, 1, 33, op) == -2
    with pytest.raises(mh.capi.MultiHError):
        engine.polish_homographies(lab, IDENT, 33)


def _host(mh):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    for fn in (host.mhh_set_tail_refit, host.mhh_set_tail_score, host.mhh_set_tail_polish, host.mhh_set_model_polish):
        fn.argtypes, fn.restype = [C.c_int], None
    return host


@pytest.mark.parametrize("refit", [0, 1])
def test_the_degenerate_tail_polishes_its_result(mh, engine_lib, synth, refit):
    """The one-plane scene of test_gpu_refit_h.test_the_degenerate_tail_refits_its_winner.  With SetTailPolish(10) Process()
    returns the labels of the run without polish and the twin's polish of that run's model over those labels — behind the
    refit (1: OpenCV's sequence) and behind the raw winner (0) —; with 0 it is that run bit for bit; 33 is refused."""
    host = _host(mh)
    sc = synth.make_scene(1500, 1, seed=41, with_neighbours=False)
    H0 = alt._initial_models(sc, 41, 1, 1)
    try:
        host.mhh_set_tail_refit(refit)
        k0, labels0, Hd, it0, en0 = alt._run_process(mh, sc, 41, H0=H0)
        host.mhh_set_tail_polish(10)
        kp, labelsp, Hp, itp, enp = alt._run_process(mh, sc, 41, H0=H0)
        host.mhh_set_tail_polish(0)
        kz, labelsz, Hz, itz, enz = alt._run_process(mh, sc, 41, H0=H0)
        host.mhh_set_tail_polish(33)
        k33 = alt._run_process(mh, sc, 41, H0=H0)[0]
    finally:
        host.mhh_set_tail_polish(-1)
        host.mhh_set_tail_refit(-1)
    assert k0 == kp == kz == 1 and k33 == -1
    assert np.array_equal(labelsp, labels0) and (itp, enp) == (it0, en0)
    H, cost, info = P.polish(sc.src, sc.dst, labels0, Hd, 10)
    assert info[0, 0] == int((labels0 == 0).sum()) and info[0, 2] >= 1, "the scene should let the polish change the model"
    assert np.array_equal(_bits(Hp), _bits(H)) and cost[0, 1] < cost[0, 0]
    assert np.array_equal(labelsz, labels0) and np.array_equal(_bits(Hz), _bits(Hd)) and (itz, enz) == (it0, en0)


def _run_points(mh, sc, seed, H0):
    """alt._run_process on the point-only route: no affinities (the hook takes Process(src, dst))."""
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    dp = C.POINTER(C.c_double)
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((1024, 9))
    it, en = C.c_int(-1), C.c_double(-1)
    src, dst, F, e2, H0c = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.F, sc.e2, H0))
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), None, sc.n, F.ctypes.data_as(dp), e2.ctypes.data_as(dp),
                             C.c_double(2.6), C.c_double(alt.THR), C.c_double(alt.LOCALITY), C.c_double(alt.LAM), 20,
                             C.c_ulonglong(seed), 0, 0, 0, H0c.ctypes.data_as(dp), H0c.shape[0], labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 1024, C.byref(it), C.byref(en), None, 0, 4)
    return k, labels, Hout[:max(k, 0)].copy(), it.value, en.value


@pytest.mark.parametrize("route", ["affinities", "points"])
def test_the_final_polish_of_process(mh, engine_lib, synth, route):
    """Three planes, Process() with SetModelPolish(10): labels, energy and iterations are those of the run without it, the
    models the twin's polish of that run's models over its labels, and no model's transfer-error sum over its members rises."""
    host = _host(mh)
    if route == "affinities":
        sc = synth.make_scene(1000, 3, seed=2, with_neighbours=False)
        H0 = alt._initial_models(sc, 2, 2, 0)
        run = lambda: alt._run_process(mh, sc, 2, H0=H0)
    else:
        sc = mh.synth.make_scene(3000, 3, seed=1234, with_neighbours=False)
        H0 = alt._initial_models(sc, 1234, 1, 0)
        run = lambda: _run_points(mh, sc, 1234, H0)
    try:
        k0, labels0, Hd, it0, en0 = run()
        host.mhh_set_model_polish(10)
        kp, labelsp, Hp, itp, enp = run()
        host.mhh_set_model_polish(33)
        k33 = run()[0]
    finally:
        host.mhh_set_model_polish(-1)
    assert k0 == kp and k0 >= 2 and k33 == -1, "the scene should leave more than one cluster"
    assert np.array_equal(labelsp, labels0) and (itp, enp) == (it0, en0)
    H, cost, info = P.polish(sc.src, sc.dst, labels0, Hd, 10)
    assert np.all(info[:, 3] == 0) and info[:, 2].sum() >= 1
    assert np.array_equal(_bits(Hp), _bits(H))
    assert np.all(cost[:, 1] <= cost[:, 0])
    for c in range(k0):
        idx = np.flatnonzero(labels0 == c)
        assert P.transfer_error_sum(sc.src, sc.dst, idx, Hp[c]) <= P.transfer_error_sum(sc.src, sc.dst, idx, Hd[c]) * (1 + 1e-12)
