"""The per-point front half (M/MultiH.cpp:786-838, :850-911, :617-644) restated as the reference writes it: full 3 x 3
matrices and library solvers everywhere the product uses a closed form (inverses of T and R T, the 6 x 6 KKT system, the
null vector of the 6 x 4 HAF matrix by an SVD of that matrix itself, the polynomial's roots by a library root finder).
It shares no line with refine.hip or oracle/mh_oracle.cpp.

Every function takes mp=False.  With mp=True the same text runs in mpmath at 50 digits (mp.matrix, mp.polyroots,
mp.svd_r, mp.lu_solve); only the CPU tests do that.  The GPU tests use the float64 path and need numpy alone.

refine() also says, per row, where float64 cannot settle a DISCRETE outcome, so that a comparison with this file may
leave the row out (a comparison of engine and oracle never does):
  undecidable      |distanceError - 1| < 1e-9; a root with 1e-12 < |im| < 1e-8; |valInf - bestS| < 1e-9 bestS; the two
                   cheapest real roots within 1e-12 of each other in cost.  At most 0.5 % of any case's rows.
  ill_conditioned  a root that moves by more than the reference's own 1e-10 test for `real` when the coefficients move by
                   1e-14 of themselves, that may be real, and whose cost can be the smallest.  Where the point pair is
                   far from the epipolar geometry compared with |e| (a d - b c small against a, b, c, d), the sextic
                   tends to the square of a quadratic squared: four roots within 1e-3 of each other next to the real axis,
                   and which of them a float64 root finder calls real is chance.  At 50 digits two of them are real and
                   one is the optimum; Durand-Kerner in FP64 (kernel and oracle) leaves |im| ~ 1e-5 on them and takes
                   another root, np.roots makes them real but misplaces them by 1e-3.  Measured: 98 of 1000 rows on
                   `unit` and 26 on `near_origin`, all but one of them gross outliers, none on the four camera cases.
                   Among the inlier rows 0.5 % holds with both flags together (asserted in test_front_half_cpu.py).

TOL (below) is how far the project's own FP64 restatement (the oracle) lies from the 50-digit result, measured on the six
geometries of epipolar_cases.py; test_front_half_cpu.py holds the oracle and this file's float64 path to it, and
test_gpu_front_half.py the kernels.
"""
from __future__ import annotations

import numpy as np

MH_REFINE_KEPT, MH_REFINE_NOT_IN_MASK, MH_REFINE_TRIANGULATION, MH_REFINE_AFFINE_TEST = 0, 1, 2, 3
DIGITS = 50


# ---- two backends with one small vocabulary: column vectors and matrices indexed [i, j] ----------------------------
class _Np:
    @staticmethod
    def mat(rows):
        return np.array(rows, dtype=np.float64)

    @staticmethod
    def col(vals):
        return np.array([[v] for v in vals], dtype=np.float64)

    mm = staticmethod(lambda a, b: a @ b)
    inv = staticmethod(np.linalg.inv)
    solve = staticmethod(np.linalg.solve)
    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def norm(v):
        return np.sqrt(sum(x * x for x in np.asarray(v).ravel()))

    @staticmethod
    def roots(high_to_low):
        """np.roots, each root then polished by two Newton steps on the polynomial itself: the companion matrix's
        eigenvalues are backward stable for the matrix, which leaves clustered roots 10-100 times further off than the
        coefficients allow."""
        c = np.trim_zeros(np.asarray(high_to_low, dtype=np.float64), "f")
        if c.size < 2:
            return []
        z = np.atleast_1d(np.roots(c)).astype(np.complex128)
        dc = np.polyder(c)
        for _ in range(2):
            with np.errstate(all="ignore"):
                step = np.polyval(c, z) / np.polyval(dc, z)
            z = np.where(np.isfinite(step), z - step, z)
        return [(v.real, v.imag) for v in z]

    @staticmethod
    def null_right(a):
        """The right singular vector of the smallest singular value (numpy orders them descending)."""
        return np.linalg.svd(a)[2][-1]

    @staticmethod
    def null_left_right(a):
        u, _, vt = np.linalg.svd(a)
        return u[:, -1], vt[-1]


class _Mp:
    def __init__(self):
        import mpmath
        self.ctx = mpmath.mp.clone()
        self.ctx.dps = DIGITS
        self.sqrt = self.ctx.sqrt

    def mat(self, rows):
        return self.ctx.matrix([[self.ctx.mpf(float(v)) if isinstance(v, (float, int, np.floating)) else v for v in r] for r in rows])

    def col(self, vals):
        return self.mat([[v] for v in vals])

    def mm(self, a, b):
        return a * b

    def inv(self, a):
        return a ** -1

    def solve(self, a, b):
        return self.ctx.lu_solve(a, b)

    def norm(self, v):
        return self.ctx.sqrt(sum(x * x for x in v))

    def roots(self, high_to_low):
        c = list(high_to_low)
        while len(c) > 1 and c[0] == 0:
            c.pop(0)
        if len(c) < 2:
            return []
        return [(z.real, z.imag) for z in self.ctx.polyroots(c, maxsteps=500, extraprec=4 * DIGITS)]

    def null_right(self, a):
        _, s, v = self.ctx.svd_r(a)                      # a = u diag(s) v, s descending
        return [v[a.cols - 1, j] for j in range(a.cols)]

    def null_left_right(self, a):
        u, s, v = self.ctx.svd_r(a, full_matrices=True)
        return [u[i, a.rows - 1] for i in range(a.rows)], [v[a.cols - 1, j] for j in range(a.cols)]


_NP = _Np()
_MP = None


def _backend(mp):
    global _MP
    if not mp:
        return _NP
    if _MP is None:
        _MP = _Mp()
    return _MP


def _f(x):
    return float(x)


def _F33(B, F):
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    return B.mat([[F[i, j] for j in range(3)] for i in range(3)])


# ---- :786-799 ------------------------------------------------------------------------------------------------------
def epipoles(F, mp=False):
    """e1, e2 with F e1 = 0, e2^T F = 0, third coordinate 1: the null vectors by an SVD of F."""
    B = _backend(mp)
    left, right = B.null_left_right(_F33(B, F))
    return (np.array([_f(right[0] / right[2]), _f(right[1] / right[2])]),
            np.array([_f(left[0] / left[2]), _f(left[1] / left[2])]))


def _root_shift(coeffs, re, im, rel=1e-14):
    """How far a root z of the polynomial moves when every coefficient changes by `rel` of itself (first order):
    rel * sum |c_k| |z|^k / |p'(z)|.  FP64 coefficients carry a few 1e-16 each and a backward-stable root finder adds as
    much again, so 1e-14 is what a float64 root may be off by; where that exceeds the reference's own 1e-10 test for
    `real` (:1156), float64 cannot settle which roots are real."""
    z = complex(re, im)
    c = [float(x) for x in coeffs]                           # high to low
    n = len(c) - 1
    mag = sum(abs(ck) * abs(z) ** (n - k) for k, ck in enumerate(c))
    dp = abs(sum((n - k) * ck * z ** (n - k - 1) for k, ck in enumerate(c[:-1])))
    return np.inf if dp == 0.0 else rel * mag / dp


# ---- :1116-1188 ----------------------------------------------------------------------------------------------------
def optimal_triangulation(F, e1, e2, p, q, mp=False, raw=False):
    """OptimalTriangulation: (ok, u, v, flags).  u, v are the corrected points (x, y; raw: homogeneous columns of the
    backend); flags holds `undecidable` and `ill_conditioned` (module docstring) and the cost `best` of the root taken."""
    B = _backend(mp)
    Fm = _F33(B, F)
    T1 = B.mat([[1, 0, -p[0]], [0, 1, -p[1]], [0, 0, 1]])
    T2 = B.mat([[1, 0, -q[0]], [0, 1, -q[1]], [0, 0, 1]])
    R1 = B.mat([[e1[0], e1[1], 0], [-e1[1], e1[0], 0], [0, 0, 1]])
    R2 = B.mat([[-e2[0], -e2[1], 0], [e2[1], -e2[0], 0], [0, 0, 1]])
    F2 = B.mm(B.mm(B.inv(T2.T), Fm), B.inv(T1))
    F3 = B.mm(B.mm(R2, F2), R1.T)
    f1 = f2 = 1                                              # the third coordinates of the normalised epipoles
    a, b, c, d = F3[1, 1], F3[1, 2], F3[2, 1], F3[2, 2]
    t6 = -a * c * f1 ** 4 * (a * d - b * c)
    t5 = (a * a + f2 * f2 * c * c) ** 2 - (a * d + b * c) * f1 ** 4 * (a * d - b * c)
    t4 = (2 * (a * a + f2 * f2 * c * c) * (2 * a * b + 2 * c * d * f2 * f2) - d * b * f1 ** 4 * (a * d - b * c)
          - 2 * a * c * f1 * f1 * (a * d - b * c))
    t3 = ((2 * a * b + 2 * c * d * f2 * f2) ** 2 + 2 * (a * a + f2 * f2 * c * c) * (b * b + f2 * f2 * d * d)
          - 2 * f1 * f1 * (a * d - b * c) * (a * d + b * c))
    t2 = (2 * (2 * a * b + 2 * c * d * f2 * f2) * (b * b + f2 * f2 * d * d) - 2 * (f1 * f1 * a * d - f1 * f1 * b * c) * b * d
          - a * c * (a * d - b * c))
    t1 = (b * b + f2 * f2 * d * d) ** 2 - (a * d + b * c) * (a * d - b * c)
    t0 = -(a * d - b * c) * b * d
    coeffs = [t6, t5, t4, t3, t2, t1, t0]
    flags = {"undecidable": False, "ill_conditioned": False, "best": None}
    if not all(np.isfinite(_f(x)) for x in coeffs):
        return False, None, None, flags                      # the reference's solvePoly is undefined here; see refine()
    best_s, best_t, second, loose = 2147483647.0, 0, None, []
    for re, im in B.roots(coeffs):
        aim = abs(_f(im))
        shift = _root_shift(coeffs, _f(re), _f(im))
        if shift > 1e-10 and aim <= 1e-10 + shift:
            loose.append(_f(re) ** 2 / (1 + _f(re) ** 2) * (1 - 1e-6))
        if 1e-12 < aim < 1e-8:
            flags["undecidable"] = True
        if aim <= 1e-10:
            t = re
            val = t * t / (1 + f1 * f1 * t * t) + ((c * t + d) * (c * t + d)) / ((a * t + b) * (a * t + b) + f2 * f2 * ((c * t + d) * (c * t + d)))
            if val < best_s:
                second, best_s, best_t = best_s, val, t
            elif second is None or val < second:
                second = val
    if second is not None and second < 2147483647.0 and abs(_f(second - best_s)) <= 1e-12 * abs(_f(best_s)):
        flags["undecidable"] = True                          # two roots of one cost: the last bit picks the point
    val_inf = 1 / (f1 * f1) + (c * c) / (a * a + f2 * f2 * c * c)
    if abs(_f(val_inf - best_s)) < 1e-9 * abs(_f(best_s)):
        flags["undecidable"] = True
    flags["best"] = _f(best_s)
    # a root that float64 may or may not call real, and whose cost (at least its first term) could be the smallest
    flags["ill_conditioned"] = any(lb <= _f(best_s) for lb in loose)
    if val_inf < best_s:
        return False, None, None, flags
    point1 = B.col([0, best_t, 1])
    line2 = B.mm(F3, point1)
    point2 = B.col([-line2[0, 0] * line2[2, 0], -line2[1, 0] * line2[2, 0], line2[0, 0] * line2[0, 0] + line2[1, 0] * line2[1, 0]])
    point2 = point2 * (1 / point2[2, 0])
    u2 = B.mm(B.inv(B.mm(R1, T1)), point1)
    v2 = B.mm(B.inv(B.mm(R2, T2)), point2)
    if raw:
        return True, u2, v2, flags
    return True, np.array([_f(u2[0, 0]), _f(u2[1, 0])]), np.array([_f(v2[0, 0]), _f(v2[1, 0])]), flags


# ---- :1092-1114 ----------------------------------------------------------------------------------------------------
def beta_scale(F, pt1, pt2, mp=False):
    """GetBetaScale; pt1, pt2 homogeneous columns of the backend."""
    B = _backend(mp)
    return _beta(B, _F33(B, F), pt1, pt2)


def _beta(B, Fm, pt1, pt2):
    l1 = B.mm(Fm.T, pt2)
    l2 = B.mm(Fm, pt1)
    x_new1 = pt1[0, 0] + 1
    y_new1 = -(l1[0, 0] * x_new1 + l1[2, 0]) / l1[1, 0]
    dx1 = B.col([x_new1, y_new1, 1]) - pt1
    dx1 = dx1 * (1 / B.norm(dx1))
    return abs(B.sqrt(l2[0, 0] * l2[0, 0] + l2[1, 0] * l2[1, 0]) /
               ((-Fm[0, 0] * dx1[1, 0] + Fm[0, 1] * dx1[0, 0]) * pt2[0, 0] +
                (-Fm[1, 0] * dx1[1, 0] + Fm[1, 1] * dx1[0, 0]) * pt2[1, 0] - Fm[2, 0] * dx1[1, 0] + Fm[2, 1] * dx1[0, 0]))


def _unit_normals(B, Fm, pt1, pt2):
    l1 = B.mm(Fm.T, pt2)
    l2 = B.mm(Fm, pt1)
    l1 = l1 * (1 / l1[2, 0])
    l2 = l2 * (1 / l2[2, 0])
    n1 = B.col([l1[0, 0], l1[1, 0]])
    n2 = B.col([l2[0, 0], l2[1, 0]])
    return n1 * (1 / B.norm(n1)), n2 * (1 / B.norm(n2))


# ---- :1057-1090 ----------------------------------------------------------------------------------------------------
def affine_consistency(F, A, pt1, pt2, mp=False):
    """GetAffineConsistency's distanceError = |A^-T n1 - beta n2|."""
    B = _backend(mp)
    Fm = _F33(B, F)
    n1, n2 = _unit_normals(B, Fm, pt1, pt2)
    beta = _beta(B, Fm, pt1, pt2)
    r1 = B.mm(B.inv(A).T, n1)
    r2 = n2 * beta
    return B.norm(r1 - r2)


# ---- :1190-1223 ----------------------------------------------------------------------------------------------------
def optimal_affinity(F, A, pt1, pt2, mp=False):
    """GetOptimalAffineTransformation: the 6 x 6 KKT system of `min |A' - A|, A'^T (beta n2) = n1`, solved as a system."""
    B = _backend(mp)
    Fm = _F33(B, F)
    n1, n2 = _unit_normals(B, Fm, pt1, pt2)
    beta = _beta(B, Fm, pt1, pt2)
    if n1[0, 0] * n2[0, 0] + n1[1, 0] * n2[1, 0] < 0:
        n2 = n2 * -1
    bx, by = -beta * n2[0, 0], -beta * n2[1, 0]
    C = B.mat([[1, 0, 0, 0, bx, 0],
               [0, 1, 0, 0, 0, bx],
               [0, 0, 1, 0, by, 0],
               [0, 0, 0, 1, 0, by],
               [bx, 0, by, 0, 0, 0],
               [0, bx, 0, by, 0, 0]])
    rhs = B.col([A[0, 0], A[0, 1], A[1, 0], A[1, 1], -n1[0, 0], -n1[1, 0]])
    x = B.solve(C, rhs)
    return [x[0, 0], x[1, 0], x[2, 0], x[3, 0]]


# ---- :850-911 and :617-644 -----------------------------------------------------------------------------------------
def haf_point(F, e2, a, p, q, locality, mp=False):
    """GetHomographyHAF for one affine correspondence and its 10-D feature: (H [9], feature [10])."""
    B = _backend(mp)
    Fm = _F33(B, F)
    a11, a12, a21, a22 = (B.mat([[v]])[0, 0] for v in a)
    x1, y1, x2, y2 = (B.mat([[v]])[0, 0] for v in (p[0], p[1], q[0], q[1]))
    ex, ey = B.mat([[e2[0]]])[0, 0], B.mat([[e2[1]]])[0, 0]
    f = [Fm[i, j] for i in range(3) for j in range(3)]
    M = B.mat([[a11 * x1 + x2 - ex, a11 * y1, a11, -f[3]],
               [a12 * x1, a12 * y1 + x2 - ex, a12, -f[4]],
               [a21 * x1 + y2 - ey, a21 * y1, a21, f[0]],
               [a22 * x1, a22 * y1 + y2 - ey, a22, f[1]],
               [ex * x1 - x2 * x1, ex * y1 - x2 * y1, ex - x2, x1 * f[3] + y1 * f[4] + f[5]],
               [ey * x1 - y2 * x1, ey * y1 - y2 * y1, ey - y2, -(x1 * f[0] + y1 * f[1] + f[2])]])
    r = B.null_right(M)
    h = [None] * 9
    h[6], h[7], h[8], lam = r[0], r[1], r[2], r[3]
    for j in range(3):
        h[3 + j] = ey * h[6 + j] - lam * f[j]
        h[j] = ex * h[6 + j] + lam * f[3 + j]
    with np.errstate(all="ignore"):
        if h[8] == 0:
            return np.full(9, np.nan), np.full(10, np.nan)
        h = [v / h[8] for v in h]
        s1, s2, s3 = h[8], h[6] + h[8], h[7] + h[8]
        feat = [h[2] / s1, (h[0] + h[2]) / s2 if s2 != 0 else float("nan"), (h[1] + h[2]) / s3 if s3 != 0 else float("nan"),
                h[5] / s1, (h[3] + h[5]) / s2 if s2 != 0 else float("nan"), (h[4] + h[5]) / s3 if s3 != 0 else float("nan"),
                x1 * locality, y1 * locality, x2 * locality, y2 * locality]
    return np.array([_f(v) for v in h]), np.array([_f(v) for v in feat])


def haf_points(F, e2, src, dst, aff, locality, mp=False):
    if len(src) == 0:
        return np.zeros((0, 9)), np.zeros((0, 10))
    out = [haf_point(F, e2, aff[i], src[i], dst[i], locality, mp) for i in range(len(src))]
    return np.stack([o[0] for o in out]).reshape(-1, 9), np.stack([o[1] for o in out]).reshape(-1, 10)


# ---- :807-838 ------------------------------------------------------------------------------------------------------
def refine(F, e1, e2, src, dst, aff, mask=None, mp=False):
    """The loop of GetFundamentalMatrixAndRefineData: keep [n], reason [n] (MH_REFINE_*), out [n, 8] (x1 y1 x2 y2 a11 a12
    a21 a22; zero where not kept; the corrected pair is there for reason 3 too), undecidable [n], ill_conditioned [n],
    cost [n] (the cost of the root taken, NaN where not triangulated).

    A row with a non-finite coordinate leaves at MH_REFINE_TRIANGULATION and one with a non-finite affinity at
    MH_REFINE_AFFINE_TEST: the reference has no defined outcome for either."""
    B = _backend(mp)
    n = len(src)
    keep, reason = np.zeros(n, np.uint8), np.full(n, MH_REFINE_NOT_IN_MASK, np.uint8)
    out, und, ill, cost = np.zeros((n, 8)), np.zeros(n, bool), np.zeros(n, bool), np.full(n, np.nan)
    for i in range(n):
        if mask is not None and not mask[i]:
            continue
        reason[i] = MH_REFINE_TRIANGULATION
        if not (np.isfinite(src[i]).all() and np.isfinite(dst[i]).all()):
            continue
        with np.errstate(all="ignore"):
            ok, u2, v2, flags = optimal_triangulation(F, e1, e2, src[i], dst[i], mp, raw=True)
            und[i], ill[i] = flags["undecidable"], flags["ill_conditioned"]
            if not ok:
                continue
            cost[i] = flags["best"]
            if not all(np.isfinite(_f(v)) for v in (u2[0, 0], u2[1, 0], v2[0, 0], v2[1, 0])):
                continue
            reason[i] = MH_REFINE_AFFINE_TEST
            out[i, :4] = _f(u2[0, 0]), _f(u2[1, 0]), _f(v2[0, 0]), _f(v2[1, 0])
            if not np.isfinite(aff[i]).all():
                continue
            A = B.mat([[aff[i][0], aff[i][1]], [aff[i][2], aff[i][3]]])
            try:
                err = affine_consistency(F, A, u2, v2, mp)
            except (np.linalg.LinAlgError, ZeroDivisionError):
                continue
            if abs(_f(err) - 1.0) < 1e-9:
                und[i] = True
            if not err <= 1.0:
                continue
            opt = optimal_affinity(F, A, u2, v2, mp)
        out[i, 4:] = [_f(v) for v in opt]
        keep[i], reason[i] = 1, MH_REFINE_KEPT
    return keep, reason, out, und, ill, cost


# ---- how far FP64 lies from the 50-digit result --------------------------------------------------------------------
def tol(measured):
    """16 x measured, floor 1e-12: kernel and oracle share their operation order and differ at most in contraction."""
    return max(16.0 * measured, 1e-12)


# Per geometry and quantity, the argument of tol() is the largest deviation of the ORACLE (oracle/mh_oracle.cpp) from the
# 50-digit pass of this file over the 1000 rows of the case's scene (epipolar_cases.SEED), excluded rows left out;
# `python tests/test_front_half_cpu.py` prints the table.  Nothing here was taken from the engine.
#   e          epipoles against the exact construction, px
#   xy         corrected coordinates, px
#   aff, H, feat   relative to the row's largest entry (H after /H[8])
#   skew       |H^T F + F^T H| / (|H| |F|) of the 50-digit H itself
#   transfer, jac  how far |H(x1) - x2| (px) and |J_H(x1) - A'| / max|A'| lie above the 50-digit H's on the same row,
#              relative to max(1, that)
#   pencil     (unit only) the same for the displacement's excess over the searched minimum
# Entries above 1e-6, explained: the per-point HAF takes the eigenvector of the 4 x 4 normal matrix (as the reference
# does, :890-893), which squares the condition of a 6 x 4 matrix whose columns differ by |e2| in scale; the SVD of the
# matrix itself (this file's float64 path) stays below 5e-9 everywhere.  With |e2| ~ 1e6 (nearly_sideways) that leaves
# 1.5e-5 of H.  The epipole is a null vector divided by its third coordinate, 1e-6 of its length there: 1.3e-3 px of 1e6.
TOL = {
    "far_right": {"e": tol(5.06e-08), "xy": tol(0.0), "aff": tol(1.21e-13), "H": tol(1.80e-07), "feat": tol(1.80e-07),
                  "skew": tol(5.06e-15), "transfer": tol(7.96e-13), "jac": tol(2.74e-10)},
    "in_image": {"e": tol(6.44e-08), "xy": tol(0.0), "aff": tol(2.89e-12), "H": tol(3.57e-08), "feat": tol(3.57e-08),
                 "skew": tol(1.35e-12), "transfer": tol(2.83e-11), "jac": tol(2.85e-10)},
    "unit": {"e": tol(1.10e-14), "xy": tol(6.11e-13), "aff": tol(8.97e-15), "H": tol(1.55e-09), "feat": tol(1.40e-09),
             "skew": tol(5.21e-16), "transfer": tol(4.98e-10), "jac": tol(3.40e-10), "pencil": tol(1.36e-11)},
    "near_origin": {"e": tol(1.78e-15), "xy": tol(1.16e-12), "aff": tol(5.70e-14), "H": tol(5.38e-13), "feat": tol(5.55e-13),
                    "skew": tol(2.13e-16), "transfer": tol(1.90e-12), "jac": tol(4.29e-12)},
    "far_left": {"e": tol(1.41e-08), "xy": tol(0.0), "aff": tol(1.26e-13), "H": tol(6.65e-08), "feat": tol(6.65e-08),
                 "skew": tol(8.98e-16), "transfer": tol(9.09e-13), "jac": tol(6.34e-10)},
    "nearly_sideways": {"e": tol(1.33e-03), "xy": tol(0.0), "aff": tol(1.16e-13), "H": tol(1.51e-05), "feat": tol(1.51e-05),
                        "skew": tol(4.89e-13), "transfer": tol(2.12e-09), "jac": tol(5.75e-08)},
}
