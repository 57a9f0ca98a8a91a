"""Reference twin of the minimal-sample (7-point) fundamental-matrix estimator: float64 numpy, LAPACK's SVD for the null
space, np.roots for the cubic.  A helper, not a test.  The engine's k_fund7 / k_ransac_stop (csrc/dlt4.hip, csrc/fund.hip)
are checked against it as SETS of F per sample: the solution set of a 7-tuple does not depend on the basis of the
two-dimensional null space, so nothing here compares null vectors or roots."""
from __future__ import annotations

import math

import numpy as np


# ---- scenes ----------------------------------------------------------------------------------------------------------
def make_scene(n, seed, noise=0.5):
    """n correspondences of a two-camera scene (pixels, 640 x 480 images): points in a box 4-8 units in front of the
    first camera, the second camera turned and moved sideways; Gaussian noise of `noise` px on both images."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(4.0, 8.0, n)], axis=1)
    K = np.array([[800.0, 0.0, 320.0], [0.0, 800.0, 240.0], [0.0, 0.0, 1.0]])
    a, b = 0.12, -0.05
    Ry = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(b), -math.sin(b)], [0.0, math.sin(b), math.cos(b)]])
    R, t = Ry @ Rx, np.array([-0.8, 0.06, 0.15])
    p1 = (K @ X.T).T
    p2 = (K @ (R @ X.T + t[:, None])).T
    src = p1[:, :2] / p1[:, 2:3] + noise * rng.standard_normal((n, 2))
    dst = p2[:, :2] / p2[:, 2:3] + noise * rng.standard_normal((n, 2))
    return np.ascontiguousarray(src), np.ascontiguousarray(dst)


def uniform_rows(n, seed):
    """n correspondences with no geometry at all: both points uniform in the image."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([0.0, 0.0]), np.array([640.0, 480.0])
    return rng.uniform(lo, hi, (n, 2)), rng.uniform(lo, hi, (n, 2))


# ---- the draws -------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample7(seed, first, m, n):
    """The engine's counter-RNG 7-tuples (csrc/dlt4.hip, sample_tuple<7, 256>): draw c of sample s gives
    r = splitmix64(seed + (s << 8) + c), index ((r >> 32) n) >> 32; duplicates inside a tuple are rejected."""
    out = np.zeros((m, 7), dtype=np.int32)
    for k in range(m):
        got = []
        for c in range(256):
            if len(got) == 7:
                break
            r = _splitmix64((seed + ((first + k) << 8) + c) & _M64)
            i = ((r >> 32) * n) >> 32
            if i not in got:
                got.append(i)
        got += [got[0]] * (7 - len(got))
        out[k] = got
    return out


# ---- the solver --------------------------------------------------------------------------------------------------------
def hartley(p):
    """Centroid to the origin, mean distance sqrt 2: the normalised points and T with p_n = T p."""
    c = p.mean(axis=0)
    s = math.sqrt(2.0) / np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    T = np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])
    return (p - c) * s, T


def null_space(src7, dst7):
    """Two orthonormal vectors spanning the null space of the 7 x 9 design matrix of the normalised points (rows
    [u x, u y, u, v x, v y, v, x, y, 1], p1 = (x, y), p2 = (u, v)), as 3 x 3 matrices, with T1 and T2."""
    a, T1 = hartley(src7)
    b, T2 = hartley(dst7)
    x, y, u, v = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones(7)], axis=1)
    Vt = np.linalg.svd(A)[2]
    return Vt[7].reshape(3, 3), Vt[8].reshape(3, 3), T1, T2


def _cubic(M0, M1, nodes):
    """Coefficients (highest first) of det(M0 + t M1) from four determinant evaluations at `nodes`."""
    vals = np.array([np.linalg.det(M0 + t * M1) for t in nodes])
    return np.linalg.solve(np.vander(np.asarray(nodes, dtype=np.float64), 4), vals)


def root_gap(coef, roots=None):
    """Scaled root gap of a cubic: min over its roots r of |p'(r)| / (max|coef| max(1, |r|)^2).  Taken over ALL three roots,
    the complex ones too: a pair that is complex by a hair is as badly conditioned — for the COUNT of real roots — as a
    real pair that is nearly double, and only the latter would show at the real roots alone."""
    r = np.roots(coef) if roots is None else roots
    dp = np.polyval(np.polyder(coef), r)
    return float(np.min(np.abs(dp) / (np.max(np.abs(coef)) * np.maximum(1.0, np.abs(r)) ** 2)))


def _finish(Fn, T1, T2):
    F = T2.T @ Fn @ T1
    F = F / np.linalg.norm(F)
    return (F if F[2, 2] >= 0.0 else -F).reshape(9)


def solve7(src7, dst7, route=0):
    """All real solutions of the 7-point problem: (k x 9 unit-norm F with F[8] >= 0, scaled root gap of the cubic).
    route 0: p(t) = det(G2 + t (G1 - G2)) fitted at t = -1, 0, 1, 2;  route 1: p(t) = det(G1 + t G2) fitted at
    t = -2, -0.5, 0.5, 2 — another cubic with other roots for the same solution set."""
    G1, G2, T1, T2 = null_space(src7, dst7)
    M0, M1, nodes = (G2, G1 - G2, (-1.0, 0.0, 1.0, 2.0)) if route == 0 else (G1, G2, (-2.0, -0.5, 0.5, 2.0))
    coef = _cubic(M0, M1, nodes)
    r = np.roots(coef)
    real = r[np.abs(r.imag) <= 1e-9 * np.maximum(1.0, np.abs(r))].real
    sols = [_finish(M0 + t * M1, T1, T2) for t in np.sort(real)]
    return np.array(sols).reshape(-1, 9), root_gap(coef, r)


def set_distance(Fa, Fb):
    """Largest distance (Frobenius) from an F of set Fa to its nearest F of set Fb; inf when Fb is empty and Fa is not."""
    if len(Fa) == 0:
        return 0.0
    if len(Fb) == 0:
        return math.inf
    d = np.linalg.norm(Fa[:, None, :] - Fb[None, :, :], axis=2)
    return float(d.min(axis=1).max())


def constraint_residuals(F, src7, dst7):
    """|det F| and the seven |p2^T F p1| of one F (9 values)."""
    Fm = F.reshape(3, 3)
    p1 = np.concatenate([src7, np.ones((7, 1))], axis=1)
    p2 = np.concatenate([dst7, np.ones((7, 1))], axis=1)
    return abs(np.linalg.det(Fm)), np.abs(np.einsum("ki,ij,kj->k", p2, Fm, p1))


# ---- scoring: the formula documented in csrc/fund.hip ------------------------------------------------------------------
def epipolar_distance(F, src, dst, metric):
    """d of every point under one F (9 values); metric 0 = Sampson, 1 = the larger squared point-to-line distance."""
    f = F
    x, y, u, v = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
    a = f[0] * x + f[1] * y + f[2]
    b = f[3] * x + f[4] * y + f[5]
    c = f[6] * x + f[7] * y + f[8]
    a2 = f[0] * u + f[3] * v + f[6]
    b2 = f[1] * u + f[4] * v + f[7]
    e = u * a + v * b + c
    with np.errstate(all="ignore"):
        if metric == 0:
            return (e * e) / (a * a + b * b + a2 * a2 + b2 * b2)
        return np.maximum((e * e) / (a2 * a2 + b2 * b2), (e * e) / (a * a + b * b))


def count_bounds(F, src, dst, thr2, metric):
    """(lo, hi): the inlier count (d < thr2) of one F with the points whose d lies within a relative 1e-9 of thr2 left
    out (lo) or all counted (hi).  A slot with a NaN gives (0, 0)."""
    if not np.all(np.isfinite(F)):
        return 0, 0
    d = epipolar_distance(F, src, dst, metric)
    near = np.abs(d - thr2) <= 1e-9 * thr2
    lo = int(np.count_nonzero((d < thr2) & ~near))
    return lo, lo + int(np.count_nonzero(near))


# ---- the stop rule -------------------------------------------------------------------------------------------------------
def ransac_stop_replay(counts, n, confidence):
    """The sequential RANSAC over the counts of S samples (S x 3, sample order): (samples_used, winning slot index
    3 s + j, its count, the smallest distance of a quotient log(1 - c) / log(1 - w^7) met on the way to an integer).
    best(s) = the largest count over the slots of samples 0..s, ties to the lowest (sample, slot); N(s) = the ceiling of
    the quotient clamped to [1, S], S at best = 0 and 1 at best = n; the first s with s + 1 >= N(s) ends the run."""
    counts = np.asarray(counts).reshape(-1, 3)
    S = counts.shape[0]
    best, win, margin = 0, 0, math.inf
    for s in range(S):
        for j in range(3):
            if counts[s, j] > best:
                best, win = int(counts[s, j]), 3 * s + j
        if best <= 0:
            need = S
        elif best >= n:
            need = 1
        else:
            w = best / n
            den = math.log1p(-(w ** 7))          # log(1 - w^7); 1 - w^7 itself rounds to 1 below w = 0.0048
            q = math.log(1.0 - confidence) / den if den < 0.0 else math.inf
            if math.isfinite(q):
                margin = min(margin, abs(q - round(q)))
            need = S if not q < S else max(1, int(math.ceil(q)))
        if s + 1 >= need:
            return s + 1, win, best, margin
    raise AssertionError("unreachable: N(s) <= S")
