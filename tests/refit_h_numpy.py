"""mh_refit_homography (include/multih_hip.h; csrc/refit_h.hip, k_refit_h) in numpy, twice.

    refit            the TWIN of the rule in the header, operation for operation, so that the kernel can be held to it bit for
                     bit: d2 from oracle_lib.residual_matrix (the forward transfer error in the reference's operation order),
                     every sum in the engine's order (thread t of 256 adds the members with index = t mod 256 in ascending
                     index from 0.0, then the binary tree 128 .. 1; vectorised over the threads), the 9 x 9 solve by
                     oracle_lib.jacobi_sym (the cyclic Jacobi the device runs), the 4-point DLT proposer's de-normalisation.
                     numpy never contracts a multiplication and an addition, and sqrt and the division round correctly.
    fit_plain        the PLAIN DEFINITION of the same fit: the 2 c x 9 design matrix of the same normalised points and
                     numpy.linalg.svd, the last right singular vector.  Shares the normalisation's formulas with the twin, not
                     its summation order, its normal matrix or its eigen-solver.

tests/test_refit_h_cpu.py holds the twin to the plain definition; tests/test_gpu_refit_h.py holds the kernel to the twin.
"""
import numpy as np

import oracle_lib as O

LANES = 256
MAX_ITERATIONS = 16
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def d2_of(src, dst, H):
    with np.errstate(all="ignore"):
        return O.residual_matrix(src, dst, np.asarray(H, np.float64).reshape(1, 9))[0]


def inlier_mask(src, dst, H, thr2):
    """S(H) as flags: d2 < thr2, strictly; False for NaN."""
    with np.errstate(all="ignore"):
        return d2_of(src, dst, H) < thr2


def strided_tree_sum(idx, terms):
    """The engine's sum of terms[j] (one row per member, K columns) for the members idx (ascending point indices): [K]."""
    idx = np.asarray(idx, dtype=np.int64)
    terms = np.asarray(terms, np.float64).reshape(idx.size, -1)
    lane = idx % LANES
    acc = np.zeros((LANES, terms.shape[1]))
    if idx.size:
        # rank of a member among the members of its lane (idx ascending: a stable sort by lane keeps the index order)
        order = np.argsort(lane, kind="stable")
        sorted_lane = lane[order]
        first = np.searchsorted(sorted_lane, np.arange(LANES))
        rank = np.empty(idx.size, dtype=np.int64)
        rank[order] = np.arange(idx.size) - first[sorted_lane]
        for step in range(int(rank.max()) + 1):
            sel = rank == step                                  # at most one member per lane
            acc[lane[sel]] = acc[lane[sel]] + terms[sel]
    s = LANES // 2
    while s >= 1:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0].copy()


def normalisation(src, dst, idx):
    """(cx1, cy1, cx2, cy2, s1, s2) of the members idx by steps 1-2 of fit(S), or None when a scale is not finite."""
    c = idx.size
    x0, y0, u0, v0 = src[idx, 0], src[idx, 1], dst[idx, 0], dst[idx, 1]
    with np.errstate(all="ignore"):
        sums = strided_tree_sum(idx, np.stack([x0, y0, u0, v0], axis=1))
        inv = 1.0 / float(c)
        cx1, cy1, cx2, cy2 = (float(v * inv) for v in sums)
        ax, ay, bx, by = x0 - cx1, y0 - cy1, u0 - cx2, v0 - cy2
        d = strided_tree_sum(idx, np.stack([np.sqrt(ax * ax + ay * ay), np.sqrt(bx * bx + by * by)], axis=1))
        s1 = float(np.sqrt(2.0) / (d[0] / float(c)))
        s2 = float(np.sqrt(2.0) / (d[1] / float(c)))
    if not (np.isfinite(s1) and np.isfinite(s2)):
        return None
    return cx1, cy1, cx2, cy2, s1, s2


def normal_matrix(G):
    """The symmetric 9 x 9 of step 4 from the 24 sums G[4, 6]."""
    M = np.zeros((9, 9))
    for k, (a, b) in enumerate(PAIRS):
        for a_, b_ in ((a, b), (b, a)):
            M[a_, b_] = M[3 + a_, 3 + b_] = G[0, k]
            M[a_, 6 + b_] = M[6 + b_, a_] = -G[1, k]
            M[3 + a_, 6 + b_] = M[6 + b_, 3 + a_] = -G[2, k]
            M[6 + a_, 6 + b_] = G[3, k]
    return M


def denormalise(g, norm):
    """Steps 6-7: T2^-1 Hn T1 by k_dlt4's steps, unit Frobenius norm, h33 >= 0; None when an entry is not finite."""
    cx1, cy1, cx2, cy2, s1, s2 = norm
    with np.errstate(all="ignore"):
        A1 = np.empty(9)
        for r in range(3):
            a, b, c = g[3 * r], g[3 * r + 1], g[3 * r + 2]
            A1[3 * r] = a * s1
            A1[3 * r + 1] = b * s1
            A1[3 * r + 2] = (c - (a * s1) * cx1) - (b * s1) * cy1
        is2 = 1.0 / s2
        Hh = np.empty(9)
        for j in range(3):
            Hh[j] = A1[j] * is2 + cx2 * A1[6 + j]
            Hh[3 + j] = A1[3 + j] * is2 + cy2 * A1[6 + j]
            Hh[6 + j] = A1[6 + j]
        fro = 0.0
        for j in range(9):
            fro = fro + Hh[j] * Hh[j]
        scl = 1.0 / np.sqrt(fro)
        if Hh[8] < 0.0:
            scl = -scl
        out = Hh * scl
    return out if np.all(np.isfinite(out)) else None


def fit(src, dst, idx, witness=None):
    """fit(S) of the header for the members idx (ascending point indices): H[9], or None when it fails.
    witness (a list): receives the eigenvalues of the normal matrix, for the conditioning witness of the tests."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size < 4:
        return None
    norm = normalisation(src, dst, idx)
    if norm is None:
        return None
    cx1, cy1, cx2, cy2, s1, s2 = norm
    with np.errstate(all="ignore"):
        x, y = (src[idx, 0] - cx1) * s1, (src[idx, 1] - cy1) * s1
        u, v = (dst[idx, 0] - cx2) * s2, (dst[idx, 1] - cy2) * s2
        p = [x, y, np.ones_like(x)]
        w = u * u + v * v
        t = [p[a] * p[b] for a, b in PAIRS]
        terms = np.stack(t + [u * tt for tt in t] + [v * tt for tt in t] + [w * tt for tt in t], axis=1)
        G = strided_tree_sum(idx, terms).reshape(4, 6)
        d, V = O.jacobi_sym(normal_matrix(G))
    if witness is not None:
        witness.append(d.copy())
    jm = 0
    for j in range(1, 9):
        if d[j] < d[jm]:
            jm = j
    return denormalise(V[:, jm].copy(), norm)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def rounds(H_in, iterations, fit_of, count_of):
    """The round rule alone, on any fit and any count: (H_out, accepted, why) with why in 'iterations', 'fit failed',
    'same bits', 'fewer inliers'.  fit_of(H) -> H or None; count_of(H) -> int."""
    cur = np.array(H_in, dtype=np.float64).reshape(9)
    n_cur, accepted = count_of(cur), 0
    for _ in range(iterations):
        cand = fit_of(cur)
        if cand is None:
            return cur, accepted, "fit failed"
        if same_bits(cand, cur):
            return cur, accepted, "same bits"
        n_cand = count_of(cand)
        if n_cand < n_cur:
            return cur, accepted, "fewer inliers"
        cur, n_cur, accepted = cand, n_cand, accepted + 1
    return cur, accepted, "iterations"


def refit(src, dst, H_in, thr2, iterations, why=None):
    """The twin of mh_refit_homography: (H_out[9], mask uint8[n], inliers, fits_accepted).  why (a list): receives what
    ended the rounds."""
    assert 0 <= iterations <= MAX_ITERATIONS
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    H, accepted, reason = rounds(H_in, iterations,
                                 lambda h: fit(src, dst, np.flatnonzero(inlier_mask(src, dst, h, thr2))),
                                 lambda h: int(inlier_mask(src, dst, h, thr2).sum()))
    if why is not None:
        why.append(reason)
    mask = inlier_mask(src, dst, H, thr2)
    return H, mask.astype(np.uint8), int(mask.sum()), accepted


# ---- the plain definition --------------------------------------------------------------------------------------------

def unit_sign(H):
    """Unit Frobenius norm, h33 >= 0: how two homographies are compared."""
    H = np.asarray(H, np.float64).reshape(9)
    H = H / np.linalg.norm(H)
    return -H if H[8] < 0 else H


def fit_plain(src, dst, idx):
    """The 2 c x 9 DLT design matrix of the same normalised points, its last right singular vector, T2^-1 Hn T1."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    cx1, cy1, cx2, cy2, s1, s2 = normalisation(src, dst, idx)
    x, y = (src[idx, 0] - cx1) * s1, (src[idx, 1] - cy1) * s1
    u, v = (dst[idx, 0] - cx2) * s2, (dst[idx, 1] - cy2) * s2
    one, zero = np.ones_like(x), np.zeros_like(x)
    r1 = np.stack([-x, -y, -one, zero, zero, zero, u * x, u * y, u], axis=1)
    r2 = np.stack([zero, zero, zero, -x, -y, -one, v * x, v * y, v], axis=1)
    A = np.concatenate([r1, r2], axis=0)
    Hn = np.linalg.svd(A, full_matrices=True)[2][-1].reshape(3, 3)
    T1 = np.array([[s1, 0, -s1 * cx1], [0, s1, -s1 * cy1], [0, 0, 1]])
    T2i = np.array([[1 / s2, 0, cx2], [0, 1 / s2, cy2], [0, 0, 1]])
    return unit_sign((T2i @ Hn @ T1).reshape(9))


# ---- scenes ---------------------------------------------------------------------------------------------------------

def plane_scene(rng, c, noise, outliers=0, H=None, size=1000.0):
    """c correspondences of one random plane with `noise` px of Gaussian noise on the targets, then `outliers` uniform
    ones, shuffled: (src[n, 2], dst[n, 2], H_true[9], is_inlier[n])."""
    if H is None:
        H = np.eye(3) + rng.normal(0, 0.08, size=(3, 3))
        H[:2, 2] = rng.uniform(-40, 40, size=2)
        H[2, :2] = rng.normal(0, 5e-5, size=2)
        H[2, 2] = 1.0
    H = np.asarray(H, np.float64).reshape(3, 3)
    n = c + outliers
    src = rng.uniform(0, size, size=(n, 2))
    q = np.concatenate([src, np.ones((n, 1))], axis=1) @ H.T
    dst = q[:, :2] / q[:, 2:3] + rng.normal(0, noise, size=(n, 2)) if noise > 0 else q[:, :2] / q[:, 2:3]
    if outliers:
        dst[c:] = rng.uniform(0, size, size=(outliers, 2))
    perm = rng.permutation(n)
    good = np.zeros(n, bool)
    good[:c] = True
    return np.ascontiguousarray(src[perm]), np.ascontiguousarray(dst[perm]), unit_sign(H.reshape(9)), good[perm]
