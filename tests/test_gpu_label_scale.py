"""mh_label_residual_quantile (csrc/label_scale.hip, k_label_quantile), mh_reweight_homographies_auto (k_autoscale_reweight_h), the
self-scaled MH_ESTIMATOR_DLT re-estimator (mh_set_estimator_reweighting_auto) and the final self-scaled refit of Process()
(MultiH::SetModelReweightAuto) on the GPU, against the numpy twin of the rules in include/multih_hip.h
(tests/label_scale_numpy.py): d2_out, H_out, gain and scale as uint64 bits, info exactly.  Every chosen case asserts that it is
what it was chosen for."""
import ctypes as C
import os

import numpy as np
import pytest

import label_scale_numpy as L
import reestimate_dlt_numpy as D
import refit_h_numpy as T
import reweight_h_numpy as W
import test_gpu_alternation as alt

pytestmark = pytest.mark.gpu
C2 = 2.2 * 2.2
C2_MAX = 2.2 * 2.2 * 81.0 / 16.0                                             # the host's upper bound: the labeling's truncation threshold
DBL_MIN = 2.2250738585072014e-308
K2 = L.KAPPA2_DEFAULT
IDENT = np.eye(3).reshape(9)
RANKS = ((0, 1), (1, 2), (3, 4), (1, 1))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _quantile_held_to_the_twin(engine, src, dst, labels, H, num, den):
    d2, info = L.quantile(src, dst, labels, H, num, den)
    gd2, ginfo = engine.label_residual_quantile(labels, H, num, den)
    assert np.array_equal(ginfo, info), (num, den, ginfo.tolist(), info.tolist())
    assert np.array_equal(_bits(gd2), _bits(d2)), (num, den, gd2, d2)
    return d2, info


def _auto_held_to_the_twin(engine, src, dst, labels, H_in, rounds, num=1, den=2, kappa2=K2, c2_min=DBL_MIN, c2_max=C2_MAX):
    H, gain, scale, info = L.reweight_auto(src, dst, labels, H_in, num, den, kappa2, c2_min, c2_max, rounds)
    gH, ggain, gscale, ginfo = engine.reweight_homographies_auto(labels, H_in, num, den, kappa2, c2_min, c2_max, rounds)
    assert np.array_equal(ginfo, info), (rounds, ginfo.tolist(), info.tolist())
    assert np.array_equal(_bits(gscale), _bits(scale)), (rounds, gscale, scale)
    assert np.array_equal(_bits(ggain), _bits(gain)), (rounds, ggain, gain)
    assert np.array_equal(_bits(gH), _bits(H)), (rounds, gH, H)
    return H, gain, scale, info


def _off_by_a_pixel(H_true, rng):
    H0 = H_true / H_true[8]
    H0[2] += rng.normal(0, 1.0)
    H0[5] += rng.normal(0, 1.0)
    return H0


def stride_case(c):
    """c members of label 0 among 30 % others (label 1 or none), interleaved: (src, dst, labels, H [2, 9])."""
    rng = np.random.default_rng(c)
    others = max(int(0.3 * c), 1)
    src, dst, H_true, good = T.plane_scene(rng, c, 0.5, outliers=others)
    labels = np.where(good, 0, np.where(rng.random(c + others) < 0.5, 1, -1)).astype(np.int32)
    return src, dst, labels, np.stack([_off_by_a_pixel(H_true, rng), IDENT])


# ---- the quantile --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [1, 2, 255, 256, 257, 513, 2000])
def test_quantile_stride_edges(engine, c):
    src, dst, labels, H = stride_case(c)
    engine.set_correspondences(src, dst)
    seen = {}
    for num, den in RANKS:
        d2, info = _quantile_held_to_the_twin(engine, src, dst, labels, H, num, den)
        assert info[0, 0] == c and info[0, 3] == 0
        seen[(num, den)] = d2[0]
    assert seen[(0, 1)] <= seen[(1, 2)] <= seen[(3, 4)] <= seen[(1, 1)] and (c < 255 or seen[(0, 1)] < seen[(1, 1)])


@pytest.mark.parametrize("n", [4096, 4097, 8193])
def test_quantile_trip_edges(engine, n):
    """for_label_members takes 16 x 256 points per trip: one trip exactly, one point into the second, one into the third.
    Sparse membership: a few members per label, the last point among them."""
    rng = np.random.default_rng(n)
    src, dst, H_true, _ = T.plane_scene(rng, n, 0.5)
    labels = np.full(n, -1, np.int32)
    pick = rng.choice(n - 1, 60, replace=False)
    labels[pick[:37]], labels[pick[37:]] = 0, 1
    labels[n - 1], labels[0] = 1, 0
    H = np.stack([_off_by_a_pixel(H_true, rng), _off_by_a_pixel(H_true, rng), IDENT])
    engine.set_correspondences(src, dst)
    for num, den in RANKS:
        d2, info = _quantile_held_to_the_twin(engine, src, dst, labels, H, num, den)
        assert info[:, 0].tolist() == [int((labels == 0).sum()), int((labels == 1).sum()), 0] and info[2, 3] == 1
    assert (labels == 1).sum() >= 2 and labels[n - 1] == 1
    # the last point decides label 1's maximum
    dst2 = dst.copy()
    dst2[n - 1] += 1e4
    engine.set_correspondences(src, dst2)
    d2, info = _quantile_held_to_the_twin(engine, src, dst2, labels, H, 1, 1)
    assert d2[1] > 1e7 and info[1, 2] == info[1, 0] - 1


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
def test_quantile_membership_edges(engine, m):
    """m models; the last label has no member (status 1, the quiet NaN) and — for m > 2 — the one before it three; labels -1, m,
    m + 5 and 2^30 belong to nobody."""
    src, dst, labels, H, full = membership_case(m)
    engine.set_correspondences(src, dst)
    for num, den in RANKS:
        d2, info = _quantile_held_to_the_twin(engine, src, dst, labels, H, num, den)
        assert info[:, 0].sum() == int(((labels >= 0) & (labels < m)).sum())
        if m > 1:
            assert info[m - 1].tolist() == [0, 0, 0, 1] and _bits(d2[m - 1]) == L.QNAN_BITS
        if m > 2:
            assert info[m - 2, 0] == 3 and info[m - 2, 3] == 0
        assert np.all(info[:full, 3] == 0)


def digit_cases():
    """(name, src, dst, H, ranks) of one label each, src = 0 under a model that carries 0 to 0, so d2 = x2^2 + y2^2."""
    rng = np.random.default_rng(77)
    out = []
    # squares exactly representable, differing only in the lowest bytes of the pattern
    j = rng.permutation(300)
    x = 1.0 + j * 2.0 ** -26
    out.append(("low bytes", np.stack([x, np.zeros(300)], axis=1), IDENT, (0, 1, 2, 149, 150, 255, 256, 298, 299)))
    # powers of two: the patterns differ only in the top bytes
    e = rng.permutation(np.arange(-500, 501, 4))
    out.append(("top bytes", np.stack([2.0 ** e, np.zeros(e.size)], axis=1), IDENT, (0, 1, e.size // 2, e.size - 2, e.size - 1)))
    # a run of 100 identical members between 50 smaller and 50 larger ones: the rank on its first, an inner and its last element
    x = np.concatenate([rng.uniform(0.1, 0.9, 50), np.full(100, 3.0), rng.uniform(5.0, 9.0, 50)])
    y = np.concatenate([np.zeros(50), np.full(100, 4.0), np.zeros(50)])
    p = rng.permutation(200)
    out.append(("run", np.stack([x[p], y[p]], axis=1), IDENT, (49, 50, 51, 100, 149, 150)))
    # one member's projective denominator is 0: its key is +inf and sorts last
    dst = np.stack([rng.uniform(1, 50, 40), rng.uniform(1, 50, 40)], axis=1)
    out.append(("inf", dst, np.array([1.0, 0, 0, 0, 1.0, 0, -1.0, 0, 1.0]), (0, 20, 38, 39)))
    return out


@pytest.mark.parametrize("case", digit_cases(), ids=lambda c: c[0])
def test_quantile_digit_edges(engine, case):
    name, dst, H, ranks = case
    c = dst.shape[0]
    dst = np.ascontiguousarray(dst)
    src = np.zeros((c, 2))
    if name == "inf":
        src[17] = (1.0, 1.0)                                                 # h6 x + h8 = 0: u = v = 1 / 0
    labels = np.zeros(c, np.int32)
    keys = L.keys_of(src, dst, np.arange(c), H)
    if name == "low bytes":
        k = np.sort(keys.view(np.uint64))
        assert np.unique(k).size == c and np.all(k >> np.uint64(40) == k[0] >> np.uint64(40)), "distinct, equal in the top three bytes"
    elif name == "top bytes":
        assert np.unique(keys.view(np.uint64) >> np.uint64(52)).size == c and np.all(keys.view(np.uint64) & np.uint64((1 << 52) - 1) == 0)
    elif name == "run":
        assert (keys == 25.0).sum() == 100 and (keys < 25.0).sum() == 50
    else:
        with np.errstate(all="ignore"):
            assert np.isinf(keys).sum() == 1 and np.isinf(T.d2_of(src, dst, H)[17]), "+inf itself, not a NaN counted as +inf"
    engine.set_correspondences(src, dst)
    for r in ranks:
        d2, info = _quantile_held_to_the_twin(engine, src, dst, labels, H, r, c - 1)
        assert info[0, 1] == r and d2[0] == np.sort(keys)[r]
        if name == "run" and 50 <= r <= 149:
            assert d2[0] == 25.0 and info[0, 2] == 50
        if name == "inf":
            assert np.isinf(d2[0]) == (r == c - 1)


# ---- the self-scaled reweighting -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [4, 5, 255, 256, 257, 513, 2000])
def test_auto_stride_edges(engine, c):
    src, dst, labels, H_in = stride_case(c)
    engine.set_correspondences(src, dst)
    seen = {r: _auto_held_to_the_twin(engine, src, dst, labels, H_in, r) for r in (0, 1, 3)}
    assert all(s[3][0, 0] == c and s[3][0, 3] == 0 for s in seen.values())
    H, gain, scale, info = seen[0]
    assert np.array_equal(_bits(H), _bits(H_in)) and info[0, 2] == 0 and gain[0, 0] == gain[0, 1] and scale[0, 0] == scale[0, 1]
    if c >= 255:
        for r in (1, 3):
            H, gain, scale, info = seen[r]
            assert info[0, 2] == r and DBL_MIN < scale[0, 1] < scale[0, 0] <= C2_MAX,(r, info[0].tolist(), scale[0].tolist())


def test_auto_clamps(engine):
    """kappa2 = 2 (an exact multiplication): 2 q below c2_min, above c2_max and exactly on either bound."""
    src, dst, labels, H_in = stride_case(300)
    engine.set_correspondences(src, dst)
    q = L.quantile(src, dst, labels, H_in, 1, 2)[0][0]
    assert q > 0 and np.isfinite(q)
    for lo, hi, want in ((4.0 * q, 8.0 * q, 4.0 * q), (q / 8, q / 4, q / 4), (2.0 * q, 3.0 * q, 2.0 * q), (q, 2.0 * q, 2.0 * q)):
        for rounds in (0, 2):
            H, gain, scale, info = _auto_held_to_the_twin(engine, src, dst, labels, H_in, rounds, kappa2=2.0, c2_min=lo, c2_max=hi)
            assert scale[0, 0] == want and lo <= scale[0, 1] <= hi
    # an overflow of kappa2 * q gives c2_max
    H, gain, scale, info = _auto_held_to_the_twin(engine, src, dst, labels, H_in, 1, kappa2=1e308, c2_min=1.0, c2_max=C2_MAX)
    assert scale[0, 0] == C2_MAX


def test_auto_zero_median(engine):
    """25 of 40 members fit exactly: the median is 0, c2 = c2_min = DBL_MIN, only the exact fits weigh — each 1.0."""
    rng = np.random.default_rng(5)
    src = rng.integers(0, 1000, size=(40, 2)).astype(np.float64)
    dst = src + np.array([5.0, -3.0])
    dst[25:] += rng.normal(0, 0.4, size=(15, 2))
    p = rng.permutation(40)
    src, dst = np.ascontiguousarray(src[p]), np.ascontiguousarray(dst[p])
    Ht = np.array([1.0, 0, 5.0, 0, 1.0, -3.0, 0, 0, 1.0])
    labels = np.zeros(40, np.int32)
    engine.set_correspondences(src, dst)
    H, gain, scale, info = _auto_held_to_the_twin(engine, src, dst, labels, Ht, 0)
    assert tuple(scale[0]) == (DBL_MIN, DBL_MIN) and tuple(info[0]) == (40, 25, 0, 0) and tuple(gain[0]) == (25.0, 25.0)
    for r in (1, 3):
        H, gain, scale, info = _auto_held_to_the_twin(engine, src, dst, labels, Ht, r)
        assert scale[0, 0] == DBL_MIN and info[0, 2] >= 1
    # three exact fits of twelve with the median still 0 (rank 0 of the minimum): fewer than four weigh, the model is kept
    dst2 = dst + 7.0
    keep = np.flatnonzero(T.d2_of(src, dst, Ht) == 0.0)[:3]
    dst2[keep] = dst[keep]
    engine.set_correspondences(src, dst2)
    H, gain, scale, info = _auto_held_to_the_twin(engine, src, dst2, labels, Ht, 3, num=0, den=1)
    assert tuple(info[0]) == (40, 3, 0, 0) and np.array_equal(_bits(H[0]), _bits(Ht)) and tuple(gain[0]) == (3.0, 3.0)


def test_auto_statuses_and_aliasing(engine, mh):
    src, dst, labels, H_in, full = membership_case(17)
    H_in = H_in.copy()
    H_in[1, 4] = np.nan
    H_in[2, 8] = np.inf
    engine.set_correspondences(src, dst)
    for r in (0, 1, 3):
        H, gain, scale, info = _auto_held_to_the_twin(engine, src, dst, labels, H_in, r)
        assert info[:, 3].tolist() == [0, 2, 2] + [0] * 12 + [1, 1] and info[15, 0] == 3 and info[16, 0] == 0
        bad = info[:, 3] != 0
        assert np.all(gain[bad] == 0.0) and np.all(scale[bad] == 0.0) and np.array_equal(_bits(H[bad]), _bits(H_in[bad]))
        assert np.all(scale[~bad] > 0.0)
    # H_out may be H_in
    want = L.reweight_auto(src, dst, labels, H_in, 1, 2, K2, DBL_MIN, C2_MAX, 3)[0]
    buf = np.ascontiguousarray(H_in.copy())
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lab = np.ascontiguousarray(labels, np.int32)
    rc = engine.lib.mh_reweight_homographies_auto(engine._h, lab.ctypes.data_as(ip), buf.ctypes.data_as(dp), 17, 1, 2, C.c_double(K2),
                                                  C.c_double(DBL_MIN), C.c_double(C2_MAX), 3, buf.ctypes.data_as(dp), None, None, None)
    assert rc == 0 and np.array_equal(_bits(buf), _bits(want))


def test_auto_early_stop(engine):
    """Exact data and c2_min far above kappa2 * median: the clamp holds c2, every weight is 1.0 to the last bit or next to it,
    and the fit of a fit is that fit again."""
    src, dst, H_true, _ = T.plane_scene(np.random.default_rng(8), 300, 0.0)
    labels = np.zeros(300, np.int32)
    engine.set_correspondences(src, dst)
    kw = dict(c2_min=C2, c2_max=2.0 * C2)
    one = _auto_held_to_the_twin(engine, src, dst, labels, H_true, 1, **kw)[0][0]
    H, gain, scale, info = _auto_held_to_the_twin(engine, src, dst, labels, one, 16, **kw)
    assert info[0, 2] < 16 and info[0, 1] == 300 and tuple(scale[0]) == (C2, C2)


@pytest.mark.parametrize("c", [5, 257, 2000])
def test_equal_bounds_are_the_fixed_scale_call_bit_for_bit(engine, c):
    src, dst, labels, H_in = stride_case(c)
    engine.set_correspondences(src, dst)
    for r in (0, 1, 3):
        fH, fgain, finfo = engine.reweight_homographies(labels, H_in, C2, r)
        for num, den, kappa2 in ((1, 2, K2), (0, 1, 1e-300), (1, 1, 1e300)):
            aH, again, ascale, ainfo = engine.reweight_homographies_auto(labels, H_in, num, den, kappa2, C2, C2, r)
            assert np.array_equal(_bits(aH), _bits(fH)) and np.array_equal(_bits(again), _bits(fgain)) and np.array_equal(ainfo, finfo)
            assert np.all(ascale[ainfo[:, 3] == 0] == C2) and np.all(ascale[ainfo[:, 3] != 0] == 0.0)
        assert finfo[0, 3] == 0 and (c < 255 or r == 0 or finfo[0, 2] >= 1)


def test_engine_state_is_untouched(engine):
    rng = np.random.default_rng(2)
    src, dst, H_true, good = T.plane_scene(rng, 1050, 1.0, outliers=450)
    labels = np.where(good, 0, -1).astype(np.int32)
    engine.set_correspondences(src, dst)

    def both():
        engine.label_residual_quantile(labels, H_true, 1, 2)
        engine.reweight_homographies_auto(labels, H_true, 1, 2, K2, DBL_MIN, C2_MAX, 3)

    def run(with_calls):
        engine.propose_dlt4(77, 0, 600)
        msac = engine.score_msac(C2)
        if with_calls:
            both()
        best_msac = engine.select_best_msac()                                # (the resident weights and counts of mh_score_msac)
        counts = engine.score(C2)
        if with_calls:
            both()
        best = engine.select_best()
        if with_calls:
            engine.reweight_homographies_auto(np.arange(1500) % 5, np.tile(H_true, (5, 1)), 1, 2, K2, DBL_MIN, C2_MAX, 2)
            engine.label_residual_quantile(np.arange(1500) % 5, np.tile(H_true, (5, 1)), 3, 4)
        return engine.model_count, engine.get_models(), counts, best, engine.score(C2), msac, best_msac

    plain, mixed = run(False), run(True)
    assert plain[0] == mixed[0] == 600 and plain[3] == mixed[3] and plain[3][1] == int(plain[2].max())
    assert np.array_equal(_bits(plain[1]), _bits(mixed[1]))
    assert np.array_equal(plain[2], mixed[2]) and np.array_equal(plain[4], mixed[4]) and np.array_equal(plain[2], plain[4])
    assert all(np.array_equal(a, b) for a, b in zip(plain[5], mixed[5])) and plain[6] == mixed[6]


def test_data_cost_and_graph_are_untouched(engine):
    sc = D.three_motions(600)
    engine.set_correspondences(sc.src, sc.dst)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    engine.set_estimator("dlt")
    engine.set_models(sc.H_true)
    cost = engine.data_cost()
    want = engine.expand()
    engine.set_models(sc.H_true)
    engine.data_cost(fetch=False)
    engine.label_residual_quantile(sc.gt_label, sc.H_true, 1, 2)
    engine.reweight_homographies_auto(sc.gt_label, sc.H_true, 1, 2, K2, DBL_MIN, C2_MAX, 3)
    got = engine.expand()                                                    # (MH_ERR_NOT_SET had a call marked the data cost stale)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    assert np.array_equal(engine.data_cost(), cost)
    assert np.array_equal(_bits(engine.get_models()), _bits(sc.H_true))


def test_error_codes(mh, engine):
    lib, h = engine.lib, engine._h
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    H, out, lab, d2 = np.tile(IDENT, (2, 1)), np.empty((2, 9)), np.zeros(50, np.int32), np.empty(2)
    Hp, op, lp, qp = H.ctypes.data_as(dp), out.ctypes.data_as(dp), lab.ctypes.data_as(ip), d2.ctypes.data_as(dp)
    quant = lambda e, labels, Hs, m, num, den, o: lib.mh_label_residual_quantile(e, labels, Hs, m, num, den, o, None)
    auto = lambda e, labels, H_in, m, num, den, k2, lo, hi, rounds, H_out: lib.mh_reweight_homographies_auto(
        e, labels, H_in, m, num, den, C.c_double(k2), C.c_double(lo), C.c_double(hi), rounds, H_out, None, None, None)
    setting = lambda e, rounds, num, den, k2, lo, hi: lib.mh_set_estimator_reweighting_auto(e, rounds, num, den, C.c_double(k2),
                                                                                          C.c_double(lo), C.c_double(hi))
    assert quant(h, lp, Hp, 1, 1, 2, qp) == -4 and auto(h, lp, Hp, 1, 1, 2, K2, 1.0, 2.0, 1, op) == -4    # MH_ERR_NOT_SET
    src, dst, _, _ = T.plane_scene(np.random.default_rng(3), 50, 0.5)
    engine.set_correspondences(src, dst)
    assert quant(h, lp, Hp, 2, 1, 2, qp) == 0 and quant(h, lp, Hp, 1, 0, 1, qp) == 0 and quant(h, lp, Hp, 1, 65536, 65536, qp) == 0
    assert quant(None, lp, Hp, 1, 1, 2, qp) == -2 and quant(h, None, Hp, 1, 1, 2, qp) == -2
    assert quant(h, lp, None, 1, 1, 2, qp) == -2 and quant(h, lp, Hp, 1, 1, 2, None) == -2
    assert quant(h, lp, Hp, 0, 1, 2, qp) == -2 and quant(h, lp, Hp, 65537, 1, 2, qp) == -2
    for num, den in ((1, 0), (0, 0), (-1, 2), (3, 2), (1, 65537), (1, -2)):
        assert quant(h, lp, Hp, 1, num, den, qp) == -2, (num, den)
        assert auto(h, lp, Hp, 1, num, den, K2, 1.0, 2.0, 1, op) == -2, (num, den)
        assert setting(h, 1, num, den, K2, 1.0, 2.0) == -2, (num, den)
    assert auto(h, lp, Hp, 2, 1, 2, K2, 1.0, 2.0, 0, op) == 0 and auto(h, lp, Hp, 2, 1, 2, K2, 1.0, 1.0, 16, op) == 0
    assert auto(h, lp, Hp, 2, 1, 2, K2, DBL_MIN, 1e300, 3, Hp) == 0          # H_out may be H_in
    assert auto(None, lp, Hp, 1, 1, 2, K2, 1.0, 2.0, 1, op) == -2 and auto(h, None, Hp, 1, 1, 2, K2, 1.0, 2.0, 1, op) == -2
    assert auto(h, lp, None, 1, 1, 2, K2, 1.0, 2.0, 1, op) == -2 and auto(h, lp, Hp, 1, 1, 2, K2, 1.0, 2.0, 1, None) == -2
    assert auto(h, lp, Hp, 0, 1, 2, K2, 1.0, 2.0, 1, op) == -2 and auto(h, lp, Hp, 65537, 1, 2, K2, 1.0, 2.0, 1, op) == -2
    assert auto(h, lp, Hp, 1, 1, 2, K2, 1.0, 2.0, -1, op) == -2 and auto(h, lp, Hp, 1, 1, 2, K2, 1.0, 2.0, 17, op) == -2
    inf, nan = float("inf"), float("nan")
    for k2, lo, hi in ((0.0, 1.0, 2.0), (-1.0, 1.0, 2.0), (inf, 1.0, 2.0), (nan, 1.0, 2.0), (K2, 0.0, 2.0), (K2, -1.0, 2.0),
                       (K2, 2.0, 1.0), (K2, 1.0, inf), (K2, nan, 2.0), (K2, 1.0, nan), (K2, inf, inf)):
        assert auto(h, lp, Hp, 1, 1, 2, k2, lo, hi, 1, op) == -2, (k2, lo, hi)
        assert setting(h, 1, 1, 2, k2, lo, hi) == -2, (k2, lo, hi)
    assert setting(None, 1, 1, 2, K2, 1.0, 2.0) == -2
    assert setting(h, -1, 1, 2, K2, 1.0, 2.0) == -2 and setting(h, 17, 1, 2, K2, 1.0, 2.0) == -2
    assert setting(h, 16, 1, 2, K2, 1.0, 2.0) == 0 and setting(h, 0, 7, 0, nan, nan, nan) == 0
    with pytest.raises(mh.capi.MultiHError):
        engine.label_residual_quantile(lab, IDENT, 3, 2)
    with pytest.raises(mh.capi.MultiHError):
        engine.reweight_homographies_auto(lab, IDENT, 1, 2, K2, 1.0, 2.0, 17)


# ---- the estimator setting and the host ----------------------------------------------------------------------------------

def test_the_estimator_setting_and_the_last_setter_decides(engine):
    src, dst, labels, H_in, full = membership_case(17)
    engine.set_correspondences(src, dst)
    engine.set_estimator("dlt")
    auto_args = (1, 2, K2, DBL_MIN, C2_MAX)

    def reestimated():
        engine.set_models(H_in)
        got = engine.reestimate(labels)
        assert np.array_equal(_bits(engine.get_models()), _bits(got))
        return got, engine.label_counts()

    want_auto, counts = L.reestimate_auto(src, dst, labels, H_in, *auto_args, 3)
    want_fixed = W.reestimate(src, dst, labels, H_in, C2, 3)[0]
    want_plain = D.reestimate(src, dst, labels, H_in)[0]
    assert not np.array_equal(_bits(want_auto[:15]), _bits(want_fixed[:15])) and not np.array_equal(_bits(want_auto[:15]), _bits(want_plain[:15]))

    engine.set_estimator_reweighting_auto(3, *auto_args)
    engine.set_correspondences(src, dst)                                     # sticky
    got, n = reestimated()
    assert np.array_equal(_bits(got), _bits(want_auto)) and np.array_equal(n, counts)
    assert np.array_equal(_bits(got), _bits(engine.reweight_homographies_auto(labels, H_in, *auto_args, 3)[0]))
    assert np.array_equal(_bits(got[15:]), _bits(H_in[15:]))
    engine.set_estimator_reweighting(3, C2)                                  # the fixed rule replaces the auto one
    got, n = reestimated()
    assert np.array_equal(_bits(got), _bits(want_fixed)) and np.array_equal(n, counts)
    engine.set_estimator_reweighting_auto(3, *auto_args)                     # ... and the other way round
    assert np.array_equal(_bits(reestimated()[0]), _bits(want_auto))
    engine.set_estimator_reweighting(0, 0.0)                                 # rounds = 0 of either setter: off altogether
    assert np.array_equal(_bits(reestimated()[0]), _bits(want_plain))
    engine.set_estimator_reweighting(3, C2)
    engine.set_estimator_reweighting_auto(0)
    assert np.array_equal(_bits(reestimated()[0]), _bits(want_plain))


def test_labeling_step_with_the_setting(engine):
    sc = D.three_motions(1200)
    engine.set_correspondences(sc.src, sc.dst)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    engine.set_estimator("dlt")
    start = np.full(sc.n, -1, np.int32)
    engine.set_models(sc.H_true)
    lab0, en0, cyc0 = engine.labeling_step(False, start)
    plain = engine.get_models()
    engine.set_estimator_reweighting_auto(3, 1, 2, K2, DBL_MIN, C2_MAX)
    engine.set_models(sc.H_true)
    lab, en, cyc = engine.labeling_step(False, start)
    assert np.array_equal(lab, lab0) and (en, cyc) == (en0, cyc0)            # the labeling is made with the standing models
    assert all((lab == k).sum() >= 100 for k in range(3))
    want, counts = L.reestimate_auto(sc.src, sc.dst, lab, sc.H_true, 1, 2, K2, DBL_MIN, C2_MAX, 3)
    assert np.array_equal(_bits(engine.get_models()), _bits(want)) and np.array_equal(engine.label_counts(), counts)
    assert not np.array_equal(_bits(plain), _bits(want))


def _host(mh):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    for fn in (host.mhh_set_model_reweight, host.mhh_set_estimator_reweight, host.mhh_set_model_reweight_auto,
               host.mhh_set_estimator_reweight_auto):
        fn.argtypes, fn.restype = [C.c_int], None
    return host


def test_the_final_self_scaled_refit_of_process(mh, engine_lib, synth):
    """Three planes, Process() with SetModelReweightAuto(3): labels, energy and iterations are those of the run without it, the
    models the twin's refit of that run's models over its labels with the host's numbers (the lower median, kappa^2 = log2(100),
    c2 in [DBL_MIN, thr^2 81/16]); 17 rounds and the fixed and the auto refit together are refused."""
    host = _host(mh)
    sc = synth.make_scene(1000, 3, seed=2, with_neighbours=False)
    H0 = alt._initial_models(sc, 2, 2, 0)
    run = lambda: alt._run_process(mh, sc, 2, H0=H0)
    try:
        k0, labels0, Hd, it0, en0 = run()
        host.mhh_set_model_reweight_auto(3)
        kr, labelsr, Hr, itr, enr = run()
        host.mhh_set_model_reweight(2)
        kboth = run()[0]
        host.mhh_set_model_reweight(-1)
        host.mhh_set_model_reweight_auto(17)
        k17 = run()[0]
        host.mhh_set_model_reweight_auto(-1)
        host.mhh_set_estimator_reweight_auto(17)
        ke17 = run()[0]
        host.mhh_set_estimator_reweight_auto(2)
        host.mhh_set_estimator_reweight(2)
        keboth = run()[0]
        host.mhh_set_estimator_reweight(-1)
        host.mhh_set_estimator_reweight_auto(-1)
        kz, labelsz, Hz, itz, enz = run()
    finally:
        for fn in (host.mhh_set_model_reweight, host.mhh_set_estimator_reweight, host.mhh_set_model_reweight_auto,
                   host.mhh_set_estimator_reweight_auto):
            fn(-1)
    assert k0 == kr == kz and k0 >= 2, "the scene should leave more than one cluster"
    assert (kboth, k17, ke17, keboth) == (-1, -1, -1, -1)
    assert np.array_equal(labelsr, labels0) and (itr, enr) == (it0, en0)
    H, gain, scale, info = L.reweight_auto(sc.src, sc.dst, labels0, Hd, 1, 2, K2, DBL_MIN, alt.THR * alt.THR * 81.0 / 16.0, 3)
    assert np.all(info[:, 3] == 0) and np.all(info[:, 2] >= 1)
    assert np.array_equal(_bits(Hr), _bits(H))
    assert np.array_equal(labelsz, labels0) and np.array_equal(_bits(Hz), _bits(Hd)) and (itz, enz) == (it0, en0)
