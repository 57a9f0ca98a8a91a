"""mh_epipoles, mh_refine_correspondences, mh_refine_points, mh_get_refine_reasons and mh_local_homographies on the six
epipolar geometries of tests/epipolar_cases.py: against the oracle bit for bit, and against the float64 path of
tests/front_half_numpy.py (the reference's own text with full matrices and library solvers, held to a 50-digit pass of
itself by tests/test_front_half_cpu.py) at front_half_numpy.TOL.

Every scene is a prefix of the case's 1000-row scene, the one TOL was measured on.  Rows the reference marks undecidable
or ill-conditioned are left out of the comparisons with the reference only, never of engine against oracle.

Rows that leave at MH_REFINE_TRIANGULATION: none exists to be listed.  With f1 = f2 = 1 the cost at t = 0 is
d^2 / (b^2 + d^2) <= 1 <= 1 + c^2 / (a^2 + c^2) = the cost at infinity, the cost is continuous in t, so its smallest
stationary value never exceeds the value at infinity and `valInf < bestS` (M/MultiH.cpp:1170) needs a root finder that
misses the best real root.  A search with the float64 reference over 1 020 000 rows (170 000 per geometry: uniform in the
region, around both epipoles at 0.01, 1 and 100 px, and second points as far from their epipolar line as from e2) found
none, so no such row is listed or asserted here.  (The oracle alone dropped 3 of those rows there, all within 0.01 px of
an epipole of `nearly_sideways`, 1e6 px out, which its own epipole misses by 1.3e-3 px; at 50 digits they triangulate
and are undecidable.)  Rows with non-finite coordinates do leave there.
"""
from __future__ import annotations

import numpy as np
import pytest

import epipolar_cases as EC
import front_half_numpy as FH
from test_front_half_cpu import LOCALITY, N, beyond, chain_residuals, rel_rows

pytestmark = pytest.mark.gpu

SHAPES = (1, 255, 256, 257, 1000)                            # the block is 256 threads
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def scene(name):
    if ("scene", name) not in _CACHE:
        _CACHE["scene", name] = EC.CASES[name].scene(N, EC.SEED)
    return _CACHE["scene", name]


def reference(name, e1, e2):
    """The float64 reference on the case's 1000 rows, no mask, with the engine's epipoles: computed once per case."""
    if ("ref", name) not in _CACHE:
        src, dst, aff, _ = scene(name)
        _CACHE["ref", name] = (bits(e1).copy(), bits(e2).copy()) + FH.refine(EC.CASES[name].F, e1, e2, src, dst, aff)
    r = _CACHE["ref", name]
    assert np.array_equal(r[0], bits(e1)) and np.array_equal(r[1], bits(e2))
    return r[2:]                                             # keep, reason, out, undecidable, ill_conditioned, cost


def masks(n):
    third = np.zeros(n, np.uint8)
    third[::3] = 1
    return (None, np.zeros(n, np.uint8), third)


def check_against_reference(name, n, mask, keep, reason, out, width):
    """keep / reason equal and coordinates (affinities) within TOL off the excluded rows.  width 8: the full form; 4:
    mh_refine_points, whose rows are kept wherever the full form's reason is 0 or 3."""
    k_r, r_r, o_r, und, ill, _ = reference(name, *_CACHE["e", name])
    k_r, r_r, o_r, ok = k_r[:n].copy(), r_r[:n].copy(), o_r[:n], ~(und | ill)[:n]
    if mask is not None:
        k_r[mask == 0], r_r[mask == 0] = 0, FH.MH_REFINE_NOT_IN_MASK
    if width == 4:
        r_r[r_r == FH.MH_REFINE_AFFINE_TEST] = FH.MH_REFINE_KEPT
        k_r = (r_r == FH.MH_REFINE_KEPT).astype(np.uint8)
    assert np.array_equal(keep[ok], k_r[ok]) and np.array_equal(reason[ok], r_r[ok]), (name, n)
    k = ok & (k_r == 1)
    if k.any():
        tol = FH.TOL[name]
        assert np.abs(out[k, :4] - o_r[k, :4]).max() <= tol["xy"], (name, n, np.abs(out[k, :4] - o_r[k, :4]).max())
        if width == 8:
            assert rel_rows(out[k, 4:], o_r[k, 4:]).max() <= tol["aff"], (name, n, rel_rows(out[k, 4:], o_r[k, 4:]).max())


@pytest.mark.parametrize("name", EC.NAMES)
def test_shapes_and_masks(name, engine, oracle):
    c = EC.CASES[name]
    src, dst, aff, _ = scene(name)
    for n in SHAPES:
        engine.set_correspondences(src[:n], dst[:n], aff[:n])
        e1, e2 = engine.epipoles(c.F)
        e1_o, e2_o = oracle.epipoles(c.F)
        assert np.array_equal(bits(e1), bits(e1_o)) and np.array_equal(bits(e2), bits(e2_o))
        assert max(np.abs(e1 - c.e1).max(), np.abs(e2 - c.e2).max()) <= FH.TOL[name]["e"]
        _CACHE["e", name] = (e1, e2)
        for mask in masks(n):
            keep, out = engine.refine_correspondences(c.F, e1, e2, mask)
            reason = engine.refine_reasons()
            keep_o, out_o, reason_o = oracle.refine_points(src[:n], dst[:n], aff[:n], c.F, e1, e2, mask, with_reasons=True)
            assert np.array_equal(keep, keep_o) and np.array_equal(reason, reason_o), (name, n)
            k = keep == 1
            assert np.array_equal(bits(out[k]), bits(out_o[k])), (name, n)
            assert np.array_equal(keep, (reason == FH.MH_REFINE_KEPT).astype(np.uint8))
            if mask is not None:
                assert (reason[mask == 0] == FH.MH_REFINE_NOT_IN_MASK).all() and (reason[mask != 0] != FH.MH_REFINE_NOT_IN_MASK).all()
            check_against_reference(name, n, mask, keep, reason, out, 8)
            # step 1 alone: the oracle's points-only form bit for bit on every row it keeps (the full form's reasons 0
            # and 3), and the full form's own first four columns where it has them (reason 0; it writes nothing at 3)
            keep4, out4 = engine.refine_points(c.F, e1, e2, mask)
            reason4 = engine.refine_reasons()
            keep4_o, out4_o, reason4_o = oracle.refine_points_only(src[:n], dst[:n], c.F, e1, e2, mask)
            assert np.array_equal(keep4, keep4_o) and np.array_equal(reason4, reason4_o), (name, n)
            assert np.array_equal(bits(out4[keep4 == 1]), bits(out4_o[keep4 == 1])), (name, n)
            assert np.isin(reason4, (0, 1, 2)).all()
            assert np.array_equal(keep4, (reason4 == FH.MH_REFINE_KEPT).astype(np.uint8))
            assert np.array_equal(bits(out4[k]), bits(out[k, :4])), (name, n)
            tri = (reason == FH.MH_REFINE_KEPT) | (reason == FH.MH_REFINE_AFFINE_TEST)
            assert (reason4[tri] == FH.MH_REFINE_KEPT).all() and np.array_equal(reason4[~tri], reason[~tri])
            check_against_reference(name, n, mask, keep4, reason4, out4, 4)


@pytest.mark.parametrize("name", EC.NAMES)
def test_sign_and_power_of_two_scale_of_F_change_no_bit(name, engine):
    """Every step is symmetric in the sign of F, and a power of two scales every intermediate exactly."""
    c = EC.CASES[name]
    src, dst, aff, _ = scene(name)
    engine.set_correspondences(src, dst, aff)
    e1, e2 = engine.epipoles(c.F)
    base = None
    for s in (1.0, -1.0, 4.0, 0.125):
        keep, out = engine.refine_correspondences(s * c.F, e1, e2)
        reason = engine.refine_reasons()
        keep4, out4 = engine.refine_points(s * c.F, e1, e2)
        reason4 = engine.refine_reasons()
        got = (keep, reason, bits(out[keep == 1]), keep4, reason4, bits(out4[keep4 == 1]))
        if base is None:
            base = got
            assert keep.sum() > 200
        for a, b in zip(base, got):
            assert np.array_equal(a, b), (name, s)


@pytest.mark.parametrize("name", EC.NAMES)
def test_local_homographies(name, engine, oracle):
    c = EC.CASES[name]
    src, dst, aff, _ = scene(name)
    engine.set_correspondences(src, dst, aff)
    e1, e2 = engine.epipoles(c.F)
    keep, out = engine.refine_correspondences(c.F, e1, e2)
    rows = np.ascontiguousarray(out[keep == 1])
    engine.set_correspondences(rows[:, :2], rows[:, 2:4], rows[:, 4:])
    engine.set_epipolar(c.F, e2)
    H, feat = engine.local_homographies(LOCALITY)
    with np.errstate(all="ignore"):
        H_o, feat_o = oracle.haf_point(rows[:, :2], rows[:, 2:4], rows[:, 4:], c.F, e2, LOCALITY)
    fin = np.isfinite(H_o).all(axis=1) & np.isfinite(feat_o).all(axis=1)
    assert fin.mean() > 0.99
    assert np.array_equal(bits(H[fin]), bits(H_o[fin])) and np.array_equal(bits(feat[fin]), bits(feat_o[fin]))
    H_r, feat_r = FH.haf_points(c.F, e2, rows[:, :2], rows[:, 2:4], rows[:, 4:], LOCALITY)
    fin &= np.isfinite(H_r).all(axis=1) & np.isfinite(feat_r).all(axis=1)
    tol = FH.TOL[name]
    assert rel_rows(H[fin], H_r[fin]).max() <= tol["H"], rel_rows(H[fin], H_r[fin]).max()
    assert rel_rows(feat[fin], feat_r[fin]).max() <= tol["feat"], rel_rows(feat[fin], feat_r[fin]).max()
    # the chain on the engine's own outputs: compatible with F whatever the affinity; maps x1 onto x2 and has A' as its
    # Jacobian as well as the reference's H on the same row does (test_front_half_cpu.beyond says where that is exact)
    skew, transfer, jac = chain_residuals(c.F, H[fin], rows[fin])
    _, transfer_r, jac_r = chain_residuals(c.F, H_r[fin], rows[fin])
    assert skew.max() <= tol["skew"], skew.max()
    assert beyond(transfer, transfer_r).max() <= tol["transfer"], beyond(transfer, transfer_r).max()
    assert beyond(jac, jac_r).max() <= tol["jac"], beyond(jac, jac_r).max()
    if name == "unit":
        assert ((transfer <= 1e-9) & (jac <= 1e-9)).sum() >= 200


@pytest.mark.parametrize("name", EC.NAMES)
def test_non_finite_rows(name, engine, oracle):
    """A NaN x1, an inf y2 and a NaN a21 among 256 good rows.  A row reported kept has finite outputs under both entry
    points; a non-finite coordinate leaves at MH_REFINE_TRIANGULATION on engine, oracle and reference; a non-finite
    affinity leaves the full form at the affine test and does not reach mh_refine_points at all."""
    c = EC.CASES[name]
    src, dst, aff, _ = (a[:259].copy() for a in scene(name))
    bad_x, bad_y, bad_a = 3, 130, 257
    src[bad_x, 0], dst[bad_y, 1], aff[bad_a, 2] = np.nan, np.inf, np.nan
    good = np.ones(259, bool)
    good[[bad_x, bad_y, bad_a]] = False
    engine.set_correspondences(src, dst, aff)
    e1, e2 = engine.epipoles(c.F)
    keep, out = engine.refine_correspondences(c.F, e1, e2)
    reason = engine.refine_reasons()
    keep4, out4 = engine.refine_points(c.F, e1, e2)
    reason4 = engine.refine_reasons()
    with np.errstate(all="ignore"):
        keep_o, out_o, reason_o = oracle.refine_points(src, dst, aff, c.F, e1, e2, with_reasons=True)
        keep_r, reason_r = FH.refine(c.F, e1, e2, src, dst, aff)[:2]
        keep4_o, out4_o, reason4_o = oracle.refine_points_only(src, dst, c.F, e1, e2)
    assert np.isfinite(out[keep == 1]).all() and np.isfinite(out4[keep4 == 1]).all()
    assert np.array_equal(keep4, keep4_o) and np.array_equal(reason4, reason4_o)
    assert np.array_equal(bits(out4[keep4 == 1]), bits(out4_o[keep4 == 1]))
    assert np.array_equal(keep, keep_o) and np.array_equal(reason, reason_o)
    assert np.array_equal(bits(out[keep == 1]), bits(out_o[keep == 1]))
    for r in (reason, reason4, reason_o, reason_r):
        assert r[bad_x] == FH.MH_REFINE_TRIANGULATION and r[bad_y] == FH.MH_REFINE_TRIANGULATION
    assert reason[bad_a] == reason_o[bad_a] == reason_r[bad_a] == FH.MH_REFINE_AFFINE_TEST
    assert keep[bad_a] == 0 and keep4[bad_a] == 1 and keep4[bad_x] == 0 and keep4[bad_y] == 0
    # the finite rows are what they are without the three: same bits
    clean = [a[:259] for a in scene(name)[:3]]
    engine.set_correspondences(*clean)
    keep_c, out_c = engine.refine_correspondences(c.F, e1, e2)
    reason_c = engine.refine_reasons()
    keep4_c, out4_c = engine.refine_points(c.F, e1, e2)
    assert np.array_equal(keep[good], keep_c[good]) and np.array_equal(reason[good], reason_c[good])
    assert np.array_equal(bits(out[good & (keep == 1)]), bits(out_c[good & (keep == 1)]))
    assert np.array_equal(keep4[good], keep4_c[good]) and np.array_equal(bits(out4[keep4 == 1]), bits(out4_c[keep4 == 1]))
