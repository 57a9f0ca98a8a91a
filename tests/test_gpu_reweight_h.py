"""mh_reweight_homographies (csrc/reweight_h.hip, k_reweight_h), the reweighted MH_ESTIMATOR_DLT re-estimator
(mh_set_estimator_reweighting) and the final reweighted refit of Process() (MultiH::SetModelReweight) on the GPU, against the
numpy twin of the rule in include/multih_hip.h (tests/reweight_h_numpy.py): H_out and gain as uint64 bits, info exactly.  The
seeds of the chosen cases were found on the CPU with the twin; every such case asserts that it is what it was chosen for."""
import ctypes as C
import os

import numpy as np
import pytest

import reestimate_dlt_numpy as D
import refit_h_numpy as T
import reweight_h_numpy as W
import test_gpu_alternation as alt

pytestmark = pytest.mark.gpu
C2 = 2.2 * 2.2
IDENT = np.eye(3).reshape(9)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _held_to_the_twin(engine, src, dst, labels, H_in, c2, rounds):
    """One call against the twin; returns the twin's (H_out, gain, info)."""
    H, gain, info = W.reweight(src, dst, labels, H_in, c2, rounds)
    gH, ggain, ginfo = engine.reweight_homographies(labels, H_in, c2, rounds)
    assert np.array_equal(ginfo, info), (rounds, ginfo.tolist(), info.tolist())
    assert np.array_equal(_bits(ggain), _bits(gain)), (rounds, ggain, gain)
    assert np.array_equal(_bits(gH), _bits(H)), (rounds, gH, H)
    return H, gain, info


def _off_by_a_pixel(H_true, rng):
    H0 = H_true / H_true[8]
    H0[2] += rng.normal(0, 1.0)
    H0[5] += rng.normal(0, 1.0)
    return H0


def stride_case(n):
    rng = np.random.default_rng(n)
    others = max(int(0.3 * n), 1)
    src, dst, H_true, good = T.plane_scene(rng, n, 0.5, outliers=others)
    labels = np.where(good, 0, np.where(rng.random(n + others) < 0.5, 1, -1)).astype(np.int32)
    return src, dst, labels, np.stack([_off_by_a_pixel(H_true, rng), IDENT])


@pytest.mark.parametrize("n", [4, 5, 255, 256, 257, 513, 2000])
def test_stride_edges(engine, n):
    """The member counts at which the 256-thread sums change shape; 30 % of the points carry another label (1: refitted too,
    from the identity) or none (-1), interleaved, so the members of a thread are not consecutive trips."""
    src, dst, labels, H_in = stride_case(n)
    engine.set_correspondences(src, dst)
    seen = {r: _held_to_the_twin(engine, src, dst, labels, H_in, C2, r) for r in (0, 1, 3, 16)}
    assert all(s[2][0, 0] == n and s[2][0, 3] == 0 for s in seen.values())
    assert np.array_equal(_bits(seen[0][0]), _bits(H_in)) and seen[0][2][0, 2] == 0 and seen[0][1][0, 0] == seen[0][1][0, 1]
    if n >= 255:
        for r in (1, 3, 16):
            H, gain, info = seen[r]
            assert info[0, 2] >= 1 and gain[0, 1] > gain[0, 0], (r, info[0].tolist(), gain[0].tolist())


def membership_case(m):
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
    return src, dst, labels, H_in, full


@pytest.mark.parametrize("m", [1, 2, 17])
def test_membership_edges(engine, m):
    """m models; the last label has no member and — for m > 2 — the one before it three; labels -1, m, m + 5 and 2^30 belong
    to nobody; labels 0 and 1 (m = 17) alternate point by point."""
    src, dst, labels, H_in, full = membership_case(m)
    engine.set_correspondences(src, dst)
    for r in (0, 1, 3):
        H, gain, info = _held_to_the_twin(engine, src, dst, labels, H_in, C2, r)
        assert info[:, 0].sum() == int(((labels >= 0) & (labels < m)).sum())
        if m > 1:
            assert tuple(info[m - 1]) == (0, 0, 0, 1) and np.array_equal(_bits(H[m - 1]), _bits(H_in[m - 1]))
        if m > 2:
            assert tuple(info[m - 2]) == (3, 0, 0, 1) and np.array_equal(_bits(H[m - 2]), _bits(H_in[m - 2]))
        assert np.all(info[:full, 3] == 0) and (r == 0 or np.all(info[:full, 2] >= 1))


def threshold_case():
    """H_in the identity, c2 = 25: 60 members displaced by small whole numbers (inside), 20 by exactly (3, 4) — d2 == c2, weight
    0, outside — and 20 by (3, 4) less one ulp of the target in one coordinate (inside, with a weight of a few ulps)."""
    rng = np.random.default_rng(9)
    src = rng.integers(100, 1000, size=(100, 2)).astype(np.float64)
    dst = src.copy()
    dst[:60] += rng.integers(-1, 2, size=(60, 2))
    dst[60:] += np.array([3.0, 4.0])
    dst[80:90, 0] = np.nextafter(dst[80:90, 0], -np.inf)
    dst[90:, 1] = np.nextafter(dst[90:, 1], -np.inf)
    perm = rng.permutation(100)
    kind = np.repeat([0, 1, 2], [60, 20, 20])[perm]
    return np.ascontiguousarray(src[perm]), np.ascontiguousarray(dst[perm]), kind


def test_the_threshold_itself(engine):
    src, dst, kind = threshold_case()
    labels = np.zeros(100, np.int32)
    d2 = T.d2_of(src, dst, IDENT)
    assert np.all(d2[kind == 1] == 25.0) and np.all(d2[kind == 2] < 25.0) and np.all(d2[kind == 2] > 24.999)
    w = W.weights(src, dst, np.arange(100), IDENT, 25.0)
    assert np.all(w[kind == 1] == 0.0) and np.all(w[kind == 2] > 0.0) and np.all(w[kind == 2] < 1e-9)
    engine.set_correspondences(src, dst)
    H, gain, info = _held_to_the_twin(engine, src, dst, labels, IDENT, 25.0, 0)
    assert tuple(info[0]) == (100, 80, 0, 0)
    for r in (1, 3):
        _held_to_the_twin(engine, src, dst, labels, IDENT, 25.0, r)


def failure_cases():
    """(name, src, dst, labels, H_in) of one label each; the model is a whole-number translation, so members on it have d2 == 0."""
    rng = np.random.default_rng(21)
    Ht = np.array([1.0, 0, 5.0, 0, 1.0, -3.0, 0, 0, 1.0])
    shift = np.array([5.0, -3.0])
    out = []
    for on in (3, 4):                                                        # a support of exactly 3 and of exactly 4 among 12 members
        src = rng.integers(0, 1000, size=(12, 2)).astype(np.float64)
        dst = src + shift
        dst[on:] += rng.uniform(30, 60, size=(12 - on, 2))
        p = rng.permutation(12)
        out.append((f"support {on}", src[p], dst[p], np.zeros(12, np.int32), Ht))
    src = rng.integers(0, 1000, size=(40, 2)).astype(np.float64)
    H_nan = Ht.copy()
    H_nan[7] = np.nan
    out.append(("nan", src, src + shift, np.zeros(40, np.int32), H_nan))
    # the support is one correspondence eight times; six members far off
    src = np.concatenate([np.tile([[320.0, 451.0]], (8, 1)), rng.integers(0, 1000, size=(6, 2)).astype(np.float64)])
    dst = src + shift
    dst[8:] += 100.0
    out.append(("one point", src, dst, np.zeros(14, np.int32), Ht))
    # collinear support
    src = np.stack([25.0 * np.arange(40), 3.0 + 0.5 * 25.0 * np.arange(40)], axis=1)
    out.append(("collinear", src, src + shift + rng.normal(0, 0.3, size=(40, 2)), np.zeros(40, np.int32), Ht))
    # no member inside c2
    src = rng.integers(0, 1000, size=(40, 2)).astype(np.float64)
    out.append(("nobody inside", src, src + shift + 50.0, np.zeros(40, np.int32), Ht))
    return out


def test_failures(engine):
    for name, src, dst, labels, H_in in failure_cases():
        src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
        engine.set_correspondences(src, dst)
        for r in (0, 1, 3):
            H, gain, info = _held_to_the_twin(engine, src, dst, labels, H_in, C2, r)
            if name == "support 3":
                assert tuple(info[0]) == (12, 3, 0, 0) and np.array_equal(_bits(H[0]), _bits(H_in)) and gain[0, 0] == gain[0, 1] == 3.0
            elif name == "support 4":
                assert info[0, 0] == 12 and info[0, 3] == 0 and (r == 0 or info[0, 2] >= 1) and gain[0, 0] == 4.0
            elif name == "nan":
                assert tuple(info[0]) == (40, 0, 0, 2) and np.array_equal(_bits(H[0]), _bits(H_in)) and tuple(gain[0]) == (0.0, 0.0)
            elif name == "one point":
                assert tuple(info[0]) == (14, 8, 0, 0) and gain[0, 0] == 8.0   # (the centroid is exact: the scales are not finite)
            elif name == "nobody inside":
                assert tuple(info[0]) == (40, 0, 0, 0) and np.array_equal(_bits(H[0]), _bits(H_in)) and tuple(gain[0]) == (0.0, 0.0)


def test_early_stop(engine):
    """Exact data: every weight is 1.0 to the last bit or next to it, and the fit of a fit is that fit again."""
    src, dst, H_true, _ = T.plane_scene(np.random.default_rng(8), 300, 0.0)
    labels = np.zeros(300, np.int32)
    engine.set_correspondences(src, dst)
    one = _held_to_the_twin(engine, src, dst, labels, H_true, C2, 1)[0][0]
    H, gain, info = _held_to_the_twin(engine, src, dst, labels, one, C2, 16)
    assert info[0, 2] < 16 and info[0, 1] == 300
    assert np.array_equal(_bits(H[0]), _bits(W.reweight(src, dst, labels, one, C2, int(info[0, 2]) + 1)[0][0]))


def test_engine_state_is_untouched(engine):
    rng = np.random.default_rng(2)
    src, dst, H_true, good = T.plane_scene(rng, 1050, 1.0, outliers=450)
    labels = np.where(good, 0, -1).astype(np.int32)
    engine.set_correspondences(src, dst)

    def run(with_refit):
        engine.propose_dlt4(77, 0, 600)
        msac = engine.score_msac(C2)
        if with_refit:
            engine.reweight_homographies(labels, H_true, C2, 3)
        best_msac = engine.select_best_msac()                                # (the resident weights and counts of mh_score_msac)
        counts = engine.score(C2)
        if with_refit:
            engine.reweight_homographies(labels, H_true, C2, 3)
        best = engine.select_best()
        if with_refit:
            engine.reweight_homographies(np.arange(1500) % 5, np.tile(H_true, (5, 1)), C2, 2)
        return engine.model_count, engine.get_models(), counts, best, engine.score(C2), msac, best_msac

    plain, mixed = run(False), run(True)
    assert plain[0] == mixed[0] == 600 and plain[3] == mixed[3] and plain[3][1] == int(plain[2].max())
    assert np.array_equal(_bits(plain[1]), _bits(mixed[1]))
    assert np.array_equal(plain[2], mixed[2]) and np.array_equal(plain[4], mixed[4]) and np.array_equal(plain[2], plain[4])
    assert all(np.array_equal(a, b) for a, b in zip(plain[5], mixed[5])) and plain[6] == mixed[6]
    assert plain[6][1] == int(plain[5][1].max())


def test_data_cost_and_graph_are_untouched(engine):
    sc = D.three_motions(600)
    engine.set_correspondences(sc.src, sc.dst)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    engine.set_estimator("dlt")
    try:
        engine.set_models(sc.H_true)
        cost = engine.data_cost()
        want = engine.expand()
        engine.set_models(sc.H_true)
        engine.data_cost(fetch=False)
        engine.reweight_homographies(sc.gt_label, sc.H_true, C2, 3)
        got = engine.expand()                                                # (MH_ERR_NOT_SET had the call marked the data cost stale)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
        assert np.array_equal(engine.data_cost(), cost)
    finally:
        engine.set_estimator("haf")


def test_error_codes(mh, engine):
    lib, h = engine.lib, engine._h
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    H, out, lab = np.tile(IDENT, (2, 1)), np.empty((2, 9)), np.zeros(50, np.int32)
    Hp, op, lp = H.ctypes.data_as(dp), out.ctypes.data_as(dp), lab.ctypes.data_as(ip)
    call = lambda e, labels, H_in, m, c2, rounds, H_out: lib.mh_reweight_homographies(e, labels, H_in, m, C.c_double(c2), rounds,
                                                                                     H_out, None, None)
    setting = lambda e, rounds, c2: lib.mh_set_estimator_reweighting(e, rounds, C.c_double(c2))
    assert call(h, lp, Hp, 1, C2, 1, op) == -4                               # MH_ERR_NOT_SET: no correspondences yet
    rng = np.random.default_rng(3)
    src, dst, _, _ = T.plane_scene(rng, 50, 0.5)
    engine.set_correspondences(src, dst)
    assert call(h, lp, Hp, 1, C2, 1, op) == 0 and call(h, lp, Hp, 2, C2, 0, op) == 0 and call(h, lp, Hp, 2, C2, 16, op) == 0
    assert call(h, lp, Hp, 2, C2, 3, Hp) == 0                                # H_out may be H_in
    assert call(None, lp, Hp, 1, C2, 1, op) == -2
    assert call(h, None, Hp, 1, C2, 1, op) == -2
    assert call(h, lp, None, 1, C2, 1, op) == -2
    assert call(h, lp, Hp, 1, C2, 1, None) == -2
    assert call(h, lp, Hp, 0, C2, 1, op) == -2 and call(h, lp, Hp, -1, C2, 1, op) == -2
    assert call(h, lp, Hp, 65537, C2, 1, op) == -2                           # (refused before anything of that size is read)
    assert call(h, lp, Hp, 1, C2, -1, op) == -2 and call(h, lp, Hp, 1, C2, 17, op) == -2
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(h, lp, Hp, 1, bad, 1, op) == -2, bad
        assert setting(h, 1, bad) == -2, bad
    assert setting(None, 1, C2) == -2
    assert setting(h, -1, C2) == -2 and setting(h, 17, C2) == -2
    assert setting(h, 16, C2) == 0 and setting(h, 0, float("nan")) == 0
    with pytest.raises(mh.capi.MultiHError):
        engine.reweight_homographies(lab, IDENT, C2, 17)


def _label_counts(engine, nh):
    out = engine.label_counts()
    assert out.shape == (nh,)
    return out


def test_the_estimator_option(engine):
    """Under "dlt" with 3 rounds mh_reestimate is mh_reweight_homographies on the resident models, in place; with 0 rounds it is
    the plain fit again; the setting survives mh_set_correspondences."""
    src, dst, labels, H_in, full = membership_case(17)
    engine.set_correspondences(src, dst)
    engine.set_estimator("dlt")
    engine.set_estimator_reweighting(3, C2)
    engine.set_correspondences(src, dst)                                     # sticky
    engine.set_models(H_in)
    got = engine.reestimate(labels)
    call = engine.reweight_homographies(labels, H_in, C2, 3)
    want, counts = W.reestimate(src, dst, labels, H_in, C2, 3)
    assert np.array_equal(_bits(got), _bits(call[0])) and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(engine.get_models()), _bits(want)) and np.array_equal(_label_counts(engine, 17), counts)
    assert np.array_equal(_bits(got[15:]), _bits(H_in[15:])) and not np.array_equal(_bits(got[:15]), _bits(H_in[:15]))
    engine.set_estimator_reweighting(0, 0.0)
    engine.set_models(H_in)
    plain = engine.reestimate(labels)
    want0, counts0 = D.reestimate(src, dst, labels, H_in)
    assert np.array_equal(_bits(plain), _bits(want0)) and np.array_equal(_label_counts(engine, 17), counts0)
    assert not np.array_equal(_bits(plain[:15]), _bits(got[:15]))


def test_labeling_step_with_the_option(engine):
    sc = D.three_motions(1200)
    engine.set_correspondences(sc.src, sc.dst)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    engine.set_estimator("dlt")
    start = np.full(sc.n, -1, np.int32)
    engine.set_models(sc.H_true)
    lab0, en0, cyc0 = engine.labeling_step(False, start)
    plain = engine.get_models()
    engine.set_estimator_reweighting(3, C2)
    engine.set_models(sc.H_true)
    lab, en, cyc = engine.labeling_step(False, start)
    assert np.array_equal(lab, lab0) and (en, cyc) == (en0, cyc0)            # the labeling is made with the standing models
    assert all((lab == k).sum() >= 100 for k in range(3))
    want, counts = W.reestimate(sc.src, sc.dst, lab, sc.H_true, C2, 3)
    assert np.array_equal(_bits(engine.get_models()), _bits(want)) and np.array_equal(_label_counts(engine, 3), counts)
    assert np.array_equal(_bits(plain), _bits(D.reestimate(sc.src, sc.dst, lab0, sc.H_true)[0]))
    assert not np.array_equal(_bits(plain), _bits(want))


def _host(mh):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    for fn in (host.mhh_set_model_reweight, host.mhh_set_estimator_reweight, host.mhh_set_model_polish):
        fn.argtypes, fn.restype = [C.c_int], None
    return host


def test_the_final_reweighted_refit_of_process(mh, engine_lib, synth):
    """Three planes, Process() with SetModelReweight(3): labels, energy and iterations are those of the run without it, the
    models the twin's refit of that run's models over its labels at the homography threshold; 17 rounds are refused, for the
    final refit and for the estimator's."""
    host = _host(mh)
    sc = synth.make_scene(1000, 3, seed=2, with_neighbours=False)
    H0 = alt._initial_models(sc, 2, 2, 0)
    run = lambda: alt._run_process(mh, sc, 2, H0=H0)
    try:
        k0, labels0, Hd, it0, en0 = run()
        host.mhh_set_model_reweight(3)
        kr, labelsr, Hr, itr, enr = run()
        host.mhh_set_model_reweight(17)
        k17 = run()[0]
        host.mhh_set_model_reweight(-1)
        host.mhh_set_estimator_reweight(17)
        ke17 = run()[0]
        host.mhh_set_estimator_reweight(-1)
        kz, labelsz, Hz, itz, enz = run()
    finally:
        host.mhh_set_model_reweight(-1)
        host.mhh_set_estimator_reweight(-1)
    assert k0 == kr == kz and k0 >= 2 and k17 == -1 and ke17 == -1, "the scene should leave more than one cluster"
    assert np.array_equal(labelsr, labels0) and (itr, enr) == (it0, en0)
    H, gain, info = W.reweight(sc.src, sc.dst, labels0, Hd, alt.THR * alt.THR, 3)
    assert np.all(info[:, 3] == 0) and np.all(info[:, 2] >= 1)
    assert np.array_equal(_bits(Hr), _bits(H))
    assert np.array_equal(labelsz, labels0) and np.array_equal(_bits(Hz), _bits(Hd)) and (itz, enz) == (it0, en0)
