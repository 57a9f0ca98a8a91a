"""The per-point front half on six epipolar geometries (tests/epipolar_cases.py), on the CPU: the oracle's restatement
of refine.hip / k_haf_point against a 50-digit transcription of the reference's own text (tests/front_half_numpy.py),
the float64 path of that transcription against the same, and the definitions themselves (the corrected pair is the
global optimum over the epipolar pencil; the per-point homography is compatible with F, maps the point and has the
optimal affinity as its Jacobian).

Every stage gets identical inputs on both sides (F and the oracle's epipoles; for HAF the oracle's refined rows), so
that a TOL entry is the error of ONE stage.  `python tests/test_front_half_cpu.py` prints the measured table behind
front_half_numpy.TOL.
"""
from __future__ import annotations

import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as EC  # noqa: E402
import front_half_numpy as FH  # noqa: E402

N = 1000
LOCALITY = 0.005
ILL_CONDITIONED = {"far_right": 0, "in_image": 0, "unit": 108, "near_origin": 29, "far_left": 0, "nearly_sideways": 0}
QUANTITIES = ("e", "xy", "aff", "H", "feat", "skew", "transfer", "jac")


def rel_rows(a, b):
    """Per row: max |a - b| over the row's largest |b|."""
    return np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)


def chain_residuals(F, H, rows):
    """Per finite H: |H^T F + F^T H| / (|H| |F|), the transfer error |H(x1) - x2| in px, and |J_H(x1) - A'| relative to
    the largest entry of A'."""
    F3 = np.asarray(F).reshape(3, 3)
    skew, transfer, jac = [], [], []
    for h, r in zip(H, rows):
        h3 = h.reshape(3, 3)
        s = h3.T @ F3 + F3.T @ h3
        skew.append(np.linalg.norm(s) / (np.linalg.norm(h3) * np.linalg.norm(F3)))
        transfer.append(np.abs(EC.apply_h(h, r[None, :2])[0] - r[2:4]).max())
        jac.append(np.abs(EC.jacobian_h(h, r[None, :2])[0] - r[4:]).max() / np.abs(r[4:]).max())
    return np.array(skew), np.array(transfer), np.array(jac)


def beyond(res, res_ref):
    """How far a chain residual lies above the 50-digit reference's on the same row, relative to max(1, reference).
    H x1 = x2 and J_H(x1) = A' are exact only where A' is consistent with F: |e1| = |e2| = 1 (elsewhere the reference's
    f1 = f2 = 1 leaves the corrected pair off the epipolar geometry) AND the sign the reference gives n2 (:1207, by
    n1 . n2 >= 0) is the true one.  Elsewhere the least-squares H has a residual of its own, the same on every side."""
    return np.maximum(res - res_ref, 0.0) / np.maximum(1.0, res_ref)


def compute(name):
    """Everything the tests of one geometry share: the scene, the oracle's outputs, and the reference's in float64 and at
    50 digits.  Runs in a worker process (the 50-digit pass takes ~20 ms a row)."""
    import oracle_lib as O
    c = EC.CASES[name]
    src, dst, aff, gt = c.scene(N, EC.SEED)
    d = {"src": src, "dst": dst, "aff": aff, "gt": gt}
    d["e_oracle"] = e1, e2 = O.epipoles(c.F)
    d["e_f64"] = FH.epipoles(c.F)
    d["e_mp"] = FH.epipoles(c.F, mp=True)
    d["oracle"] = O.refine_points(src, dst, aff, c.F, e1, e2, with_reasons=True)          # keep, out, reason
    d["f64"] = FH.refine(c.F, e1, e2, src, dst, aff)                                      # keep, reason, out, und, ill, cost
    d["mp"] = FH.refine(c.F, e1, e2, src, dst, aff, mp=True)
    rows = d["oracle"][1][d["oracle"][0] == 1]
    d["rows"] = rows
    with np.errstate(all="ignore"):
        d["haf_oracle"] = O.haf_point(rows[:, :2], rows[:, 2:4], rows[:, 4:], c.F, e2, LOCALITY)
    d["haf_f64"] = FH.haf_points(c.F, e2, rows[:, :2], rows[:, 2:4], rows[:, 4:], LOCALITY)
    d["haf_mp"] = FH.haf_points(c.F, e2, rows[:, :2], rows[:, 2:4], rows[:, 4:], LOCALITY, mp=True)
    return name, d


_DATA = {}


def data(name):
    if not _DATA:
        import multiprocessing
        import oracle_lib
        oracle_lib.lib()                                     # built once, here: the workers only load it
        with ProcessPoolExecutor(max_workers=min(len(EC.NAMES), os.cpu_count() or 1),
                                 mp_context=multiprocessing.get_context("spawn")) as pool:
            _DATA.update(dict(pool.map(compute, EC.NAMES)))
    return _DATA[name]


def excluded(d):
    """Rows left out of every comparison with the reference (never of engine against oracle): the undecidable ones and
    those whose root cluster float64 cannot resolve, by the float64 or the 50-digit pass."""
    return d["f64"][3] | d["mp"][3] | d["f64"][4] | d["mp"][4]


def deviations(name, side):
    """The largest deviation of `side` ("oracle" or "f64") from the 50-digit reference, per quantity."""
    c, d = EC.CASES[name], data(name)
    if side == "oracle":
        keep, out, reason = d["oracle"]
    else:
        keep, reason, out = d["f64"][:3]
    km, rm, om = d["mp"][:3]
    ok = ~excluded(d)
    assert np.array_equal(keep[ok], km[ok]) and np.array_equal(reason[ok], rm[ok]), name
    tri = ok & (rm != FH.MH_REFINE_TRIANGULATION)            # rows with a corrected pair on both sides: reason 0 or 3
    k = ok & (km == 1)
    if side == "oracle":
        tri = k                                              # the oracle zeroes the rows it does not keep
    H, feat = d["haf_" + side]
    Hm, featm = d["haf_mp"]
    fin = np.isfinite(H).all(axis=1) & np.isfinite(Hm).all(axis=1) & np.isfinite(feat).all(axis=1)
    skew, transfer, jac = chain_residuals(c.F, H[fin], d["rows"][fin])
    _, transfer_m, jac_m = chain_residuals(c.F, Hm[fin], d["rows"][fin])
    e = d["e_" + side]
    return {"e": max(np.abs(e[0] - c.e1).max(), np.abs(e[1] - c.e2).max()),
            "xy": np.abs(out[tri, :4] - om[tri, :4]).max(),
            "aff": rel_rows(out[k, 4:], om[k, 4:]).max(),
            "H": rel_rows(H[fin], Hm[fin]).max(),
            "feat": rel_rows(feat[fin], featm[fin]).max(),
            "skew": skew.max(), "transfer": beyond(transfer, transfer_m).max(), "jac": beyond(jac, jac_m).max()}


@pytest.mark.parametrize("name", EC.NAMES)
def test_cases_are_what_they_say(name, mh):
    c = EC.CASES[name]
    F = c.F.reshape(3, 3)
    assert abs(np.linalg.norm(F) - 1.0) < 1e-15
    scale = max(1.0, np.abs(c.e1).max(), np.abs(c.e2).max())
    assert np.abs(F @ [c.e1[0], c.e1[1], 1.0]).max() < 1e-14 * scale
    assert np.abs(F.T @ [c.e2[0], c.e2[1], 1.0]).max() < 1e-14 * scale
    src, dst, aff, gt = c.scene(N, EC.SEED)
    assert src.min() >= c.lo and src.max() <= c.hi and abs((gt < 0).mean() - EC.OUTLIERS) < 0.04
    # the generated inliers obey F: the planes are compatible with it
    x1 = np.concatenate([src, np.ones((N, 1))], axis=1)
    x2 = np.concatenate([dst, np.ones((N, 1))], axis=1)
    l2 = x1 @ F.T
    dist = np.abs((x2 * l2).sum(axis=1)) / np.hypot(l2[:, 0], l2[:, 1])
    near = np.zeros(N, bool)
    near[N - c.near_epipole_rows:] = c.near_epipole_rows > 0
    assert np.median(dist[(gt >= 0) & ~near]) < 2.0 * c.noise
    if name == "far_right":                                  # the control IS synth's geometry
        sc = mh.synth.make_scene(16, 2, seed=1, with_neighbours=False)
        assert np.allclose(sc.F, c.F, rtol=0, atol=1e-15) and np.allclose(sc.e2, c.e2, rtol=1e-14)
    if name == "in_image":
        k = c.near_epipole_rows
        assert k == 8 and (np.hypot(*(src[N - k:N - k // 2] - c.e1).T) <= 1.0).all()
        assert (np.hypot(*(dst[N - k // 2:] - c.e2).T) <= 1.0).all()


@pytest.mark.parametrize("name", EC.NAMES)
def test_at_most_half_a_percent_undecidable(name):
    """The four criteria of `undecidable` mark at most 0.5 % of the rows of any case.  `ill_conditioned` (see
    front_half_numpy) marks gross outliers only: with it, 0.5 % still holds over the inlier rows; it marks no row of a
    camera case, and on `unit` and `near_origin` no more than measured (98 and 26 of 1000, plus a tenth)."""
    d = data(name)
    und, ill = d["f64"][3] | d["mp"][3], d["f64"][4] | d["mp"][4]
    print(name, "undecidable", int(und.sum()), "ill-conditioned", int(ill.sum()), "of them inliers", int(ill[d["gt"] >= 0].sum()))
    assert und.mean() <= 0.005
    assert (und | ill)[d["gt"] >= 0].mean() <= 0.005
    assert ill.sum() <= ILL_CONDITIONED[name]


@pytest.mark.parametrize("side", ["oracle", "f64"])
@pytest.mark.parametrize("name", EC.NAMES)
def test_against_the_50_digit_reference(name, side):
    """keep and reason equal off the undecidable rows; epipoles, coordinates, affinities, H, features and the chain's
    three properties within TOL."""
    dev = deviations(name, side)
    print(name, side, {q: f"{v:.2e}" for q, v in dev.items()})
    for q in QUANTITIES:
        assert dev[q] <= FH.TOL[name][q], (name, side, q, dev[q], FH.TOL[name][q])


def test_the_chain_is_exact_where_its_premises_hold():
    """On `unit`, wherever the reference's sign of n2 is the true one, the per-point homography maps x1 onto x2 and has
    the optimal affinity as its Jacobian to rounding: that is most of the kept rows, so the row-by-row bound of
    test_against_the_50_digit_reference is not a comparison of two large residuals."""
    d = data("unit")
    for side in ("oracle", "f64", "mp"):
        H, _ = d["haf_" + side]
        _, transfer, jac = chain_residuals(EC.CASES["unit"].F, H, d["rows"])
        exact = (transfer <= 1e-9) & (jac <= 1e-9)
        print(side, int(exact.sum()), "of", len(exact))
        assert exact.sum() >= 200 and exact.mean() >= 0.75


def pencil_minimum(F, e1, p, q, steps=20000):
    """The smallest summed squared distance of p and q to a pair of corresponding epipolar lines, by search: the line
    through e1 at angle theta, its image under F, a grid of `steps` angles over [0, pi) and a bounded scalar refinement
    around the best one.  Nothing of OptimalTriangulation's algebra is used."""
    from scipy.optimize import minimize_scalar
    F3 = np.asarray(F).reshape(3, 3)

    def cost(theta, p, q):
        dx, dy = np.cos(theta), np.sin(theta)
        d1 = -dy * (p[..., 0] - e1[0]) + dx * (p[..., 1] - e1[1])
        l = F3[:, 0] * np.expand_dims(dx, -1) + F3[:, 1] * np.expand_dims(dy, -1)      # F (dx, dy, 0): F e1 = 0
        d2 = (l[..., 0] * q[..., 0] + l[..., 1] * q[..., 1] + l[..., 2]) ** 2 / (l[..., 0] ** 2 + l[..., 1] ** 2)
        return d1 * d1 + d2

    grid = np.arange(steps) * (np.pi / steps)
    best = np.empty(len(p))
    for i in range(len(p)):
        j = int(np.argmin(cost(grid, p[i], q[i])))
        r = minimize_scalar(lambda th: float(cost(np.float64(th), p[i], q[i])), method="bounded",
                            bounds=(grid[j] - np.pi / steps, grid[j] + np.pi / steps), options={"xatol": 1e-13})
        best[i] = min(r.fun, cost(grid[j], p[i], q[i]))
    return best


def displacement(out, src, dst):
    return ((out[:, :2] - src) ** 2).sum(axis=1) + ((out[:, 2:4] - dst) ** 2).sum(axis=1)


def definitions(side):
    """On `unit`, per row (NaN where `side` has no corrected pair or the row is excluded): the epipolar residual of the
    corrected pair relative to |x1'| |x2'|, and how far its summed squared displacement lies above the searched minimum,
    relative to that minimum.  side: oracle, f64 or mp."""
    c, d = EC.CASES["unit"], data("unit")
    if side == "oracle":
        keep, out, _ = d["oracle"]
        rows = keep == 1
    else:
        _, reason, out = d[side][:3]
        rows = (reason == FH.MH_REFINE_KEPT) | (reason == FH.MH_REFINE_AFFINE_TEST)
    rows = rows & ~excluded(d)
    x1 = np.concatenate([out[:, :2], np.ones((N, 1))], axis=1)
    x2 = np.concatenate([out[:, 2:4], np.ones((N, 1))], axis=1)
    epi = np.abs(((x2 @ c.F.reshape(3, 3)) * x1).sum(axis=1)) / (np.linalg.norm(x1, axis=1) * np.linalg.norm(x2, axis=1))
    if "pencil" not in d:
        d["pencil"] = pencil_minimum(c.F, c.e1, d["src"], d["dst"])
    above = displacement(out, d["src"], d["dst"]) / d["pencil"] - 1.0
    return np.where(rows, epi, np.nan), np.where(rows, above, np.nan)


def test_definitions_on_unit():
    """|e1| = |e2| = 1, so R1 and R2 are rotations and the back-mapping is the inverse of the forward one: the corrected
    pair satisfies the epipolar constraint to rounding.  It is NOT the closest such pair, not even at 50 digits: the
    reference rotates by the epipole's own direction, not by the direction from the point to the epipole (its R1, R2 are
    built once, :801-802, before any point is known), and takes (0, t) for the corrected point where Hartley and Sturm
    take the foot of the perpendicular.  Measured on this scene, the 50-digit pair's summed squared displacement lies
    between 4.5e-6 and 11 times the minimum ABOVE the minimum (median 0.013).  So the assertion is: never below the
    searched minimum (no pair on corresponding epipolar lines can be), and no further above it than the 50-digit
    reference on the same row."""
    epi_m, above_m = definitions("mp")
    assert np.nanmin(above_m) >= -1e-9
    for side in ("oracle", "f64"):
        epi, above = definitions(side)
        rows = ~np.isnan(above)
        print(side, int(rows.sum()), "rows: epipolar", epi[rows].max(), "above the searched minimum", above[rows].min(), above[rows].max(),
              "beyond the reference", (above - above_m)[rows].max())
        assert rows.sum() >= 200
        assert epi[rows].max() <= 1e-9
        assert above[rows].min() >= -1e-9
        assert (above - above_m)[rows].max() <= FH.TOL["unit"]["pencil"]


if __name__ == "__main__":
    for nm in EC.NAMES:
        dd = data(nm)
        print(nm, "undecidable f64/mp", int(dd["f64"][3].sum()), int(dd["mp"][3].sum()), "ill f64/mp/both/inliers", int(dd["f64"][4].sum()),
              int(dd["mp"][4].sum()), int((dd["f64"][4] | dd["mp"][4]).sum()), int((dd["f64"][4] | dd["mp"][4])[dd["gt"] >= 0].sum()), "kept", int(dd["mp"][0].sum()),
              "reasons", np.bincount(dd["mp"][1], minlength=4))
        for sd in ("oracle", "f64"):
            print("   %-7s" % sd, "  ".join(f"{q} {v:.2e}" for q, v in deviations(nm, sd).items()))
        Hm, _ = dd["haf_mp"]
        fin = np.isfinite(Hm).all(axis=1)
        print("   mp     ", "  ".join(f"{q} {v.max():.2e}" for q, v in zip(("skew", "transfer", "jac"), chain_residuals(EC.CASES[nm].F, Hm[fin], dd["rows"][fin]))))
    ep_m, ab_m = definitions("mp")
    print("unit definitions mp: rows %d  epipolar %.2e  above the minimum min %.2e median %.2e max %.2e" % (
        (~np.isnan(ab_m)).sum(), np.nanmax(ep_m), np.nanmin(ab_m), np.nanmedian(ab_m), np.nanmax(ab_m)))
    for sd in ("oracle", "f64"):
        ep, ab = definitions(sd)
        print("unit definitions %-7s rows %d  epipolar %.2e  pencil %.2e" % (sd, (~np.isnan(ab)).sum(), np.nanmax(ep), np.nanmax(np.abs(ab - ab_m))))
    dd = data("unit")
    Hm, _ = dd["haf_mp"]
    _, tr, jc = chain_residuals(EC.CASES["unit"].F, Hm, dd["rows"])
    print("unit: rows whose 50-digit H maps x1 onto x2 and has A' as its Jacobian to 1e-9:", int(((tr <= 1e-9) & (jc <= 1e-9)).sum()), "of", len(tr))
