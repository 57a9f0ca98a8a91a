"""mh_reweight_homographies (include/multih_hip.h; csrc/reweight_h.hip, k_reweight_h) in numpy, twice.

    reweight         the TWIN of the rule in the header, operation for operation, so that the kernel can be held to it bit for
                     bit: d2 from refit_h_numpy.d2_of (the forward transfer error in the reference's operation order), the
                     weight 1.0 - (d2 / c2), every sum in the engine's order (refit_h_numpy.strided_tree_sum over the members
                     with w > 0: the others add no term), the solve and the de-normalisation of refit_h_numpy.fit.
    wfit_plain       the PLAIN DEFINITION of one weighted fit: the 2 c x 9 design matrix of the weighted-normalised points, its
                     rows scaled by sqrt(w), and numpy.linalg.eigh of its Gram matrix.  Shares the normalisation's formulas
                     with the twin, not its summation order, its 24 sums or its eigen-solver.

tests/test_reweight_h_cpu.py holds the twin to the plain definition; tests/test_gpu_reweight_h.py holds the kernel to the twin.
"""
import numpy as np

import oracle_lib as O
import refit_h_numpy as R

MAX_ROUNDS = 16
MAX_MODELS = 65536


def weights(src, dst, idx, H, c2):
    """w of the members idx under H: d2 < c2 ? 1.0 - (d2 / c2) : 0.0; 0 for a NaN.  The support is w > 0."""
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size == 0:
        return np.zeros(0)
    with np.errstate(all="ignore"):
        d2 = R.d2_of(np.asarray(src, np.float64)[idx], np.asarray(dst, np.float64)[idx], H)
        inside = d2 < c2
        w = np.where(inside, 1.0 - (d2 / c2), 0.0)
    assert np.array_equal(w > 0.0, inside), "every member of the support has a positive weight"
    return w


def normalisation_w(src, dst, idx, w):
    """(cx1, cy1, cx2, cy2, s1, s2) of the members idx (all with w > 0) by steps 1-3 of wfit, or None when a scale is not finite."""
    x0, y0, u0, v0 = src[idx, 0], src[idx, 1], dst[idx, 0], dst[idx, 1]
    with np.errstate(all="ignore"):
        sums = R.strided_tree_sum(idx, np.stack([w * x0, w * y0, w * u0, w * v0, w], axis=1))
        W = float(sums[4])
        inv = 1.0 / W
        cx1, cy1, cx2, cy2 = (float(v * inv) for v in sums[:4])
        ax, ay, bx, by = x0 - cx1, y0 - cy1, u0 - cx2, v0 - cy2
        d = R.strided_tree_sum(idx, np.stack([w * np.sqrt(ax * ax + ay * ay), w * np.sqrt(bx * bx + by * by)], axis=1))
        s1 = float(np.sqrt(2.0) / (d[0] / W))
        s2 = float(np.sqrt(2.0) / (d[1] / W))
    if not (np.isfinite(s1) and np.isfinite(s2)):
        return None
    return cx1, cy1, cx2, cy2, s1, s2


def wfit(src, dst, idx, w):
    """wfit of the header for the members idx (ascending point indices) with the weights w: H[9], or None when it fails."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    idx, w = np.asarray(idx, dtype=np.int64), np.asarray(w, np.float64)
    keep = w > 0.0                                              # members with w == 0 add no term
    idx, w = idx[keep], w[keep]
    if idx.size < 4:
        return None
    norm = normalisation_w(src, dst, idx, w)
    if norm is None:
        return None
    cx1, cy1, cx2, cy2, s1, s2 = norm
    with np.errstate(all="ignore"):
        x, y = (src[idx, 0] - cx1) * s1, (src[idx, 1] - cy1) * s1
        u, v = (dst[idx, 0] - cx2) * s2, (dst[idx, 1] - cy2) * s2
        p = [x, y, np.ones_like(x)]
        q = u * u + v * v
        wt = [w * (p[a] * p[b]) for a, b in R.PAIRS]
        terms = np.stack(wt + [u * t for t in wt] + [v * t for t in wt] + [q * t for t in wt], axis=1)
        G = R.strided_tree_sum(idx, terms).reshape(4, 6)
        d, V = O.jacobi_sym(R.normal_matrix(G))
    jm = 0
    for j in range(1, 9):
        if d[j] < d[jm]:
            jm = j
    return R.denormalise(V[:, jm].copy(), norm)


def gain_of(idx, w):
    """(W, |support|) of the members idx with the weights w: W in the engine's order over the members with w > 0."""
    keep = w > 0.0
    if not keep.any():
        return 0.0, 0
    return float(R.strided_tree_sum(idx[keep], w[keep].reshape(-1, 1))[0]), int(keep.sum())


def reweight_one(src, dst, idx, H_in, c2, rounds):
    """One label: (H_out[9], (W_in, W_out), (members, support, done, status))."""
    H_in = np.array(H_in, dtype=np.float64).reshape(9)
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size < 4:
        return H_in.copy(), (0.0, 0.0), (int(idx.size), 0, 0, 1)
    if not np.all(np.isfinite(H_in)):
        return H_in.copy(), (0.0, 0.0), (int(idx.size), 0, 0, 2)
    cur, done = H_in.copy(), 0
    w = weights(src, dst, idx, cur, c2)
    W_in = gain_of(idx, w)[0]
    for _ in range(rounds):
        cand = wfit(src, dst, idx, w)
        if cand is None or R.same_bits(cand, cur):
            break
        cur, done = cand, done + 1
        w = weights(src, dst, idx, cur, c2)
    W_out, support = gain_of(idx, w)
    return cur, (W_in, W_out), (int(idx.size), support, done, 0)


def reweight(src, dst, labels, H_in, c2, rounds):
    """The twin of mh_reweight_homographies: (H_out [m, 9], gain [m, 2], info int32 [m, 4])."""
    assert 0 <= rounds <= MAX_ROUNDS and np.isfinite(c2) and c2 > 0
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    labels = np.asarray(labels)
    H_in = np.array(H_in, dtype=np.float64).reshape(-1, 9)
    m = H_in.shape[0]
    H, gain, info = np.empty((m, 9)), np.empty((m, 2)), np.empty((m, 4), dtype=np.int32)
    for k in range(m):
        H[k], gain[k], info[k] = reweight_one(src, dst, np.flatnonzero(labels == k), H_in[k], c2, rounds)
    return H, gain, info


def reestimate(src, dst, labels, H_in, c2, rounds):
    """MH_ESTIMATOR_DLT under mh_set_estimator_reweighting(rounds, c2), rounds >= 1: (H [Nh, 9], counts [Nh])."""
    H, _, info = reweight(src, dst, labels, H_in, c2, rounds)
    return H, info[:, 0].copy()


# ---- the plain definition --------------------------------------------------------------------------------------------

def wfit_plain(src, dst, idx, w):
    """The weighted design matrix of the weighted-normalised points (rows times sqrt(w)), the eigenvector of the smallest
    eigenvalue of its Gram matrix by numpy.linalg.eigh, T2^-1 Hn T1; unit norm, h33 >= 0."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    idx, w = np.asarray(idx, dtype=np.int64), np.asarray(w, np.float64)
    keep = w > 0.0
    idx, w = idx[keep], w[keep]
    cx1, cy1, cx2, cy2, s1, s2 = normalisation_w(src, dst, idx, w)
    x, y = (src[idx, 0] - cx1) * s1, (src[idx, 1] - cy1) * s1
    u, v = (dst[idx, 0] - cx2) * s2, (dst[idx, 1] - cy2) * s2
    one, zero = np.ones_like(x), np.zeros_like(x)
    r1 = np.stack([-x, -y, -one, zero, zero, zero, u * x, u * y, u], axis=1)
    r2 = np.stack([zero, zero, zero, -x, -y, -one, v * x, v * y, v], axis=1)
    A = np.concatenate([r1, r2], axis=0) * np.sqrt(np.concatenate([w, w]))[:, None]
    Hn = np.linalg.eigh(A.T @ A)[1][:, 0].reshape(3, 3)
    T1 = np.array([[s1, 0, -s1 * cx1], [0, s1, -s1 * cy1], [0, 0, 1]])
    T2i = np.array([[1 / s2, 0, cx2], [0, 1 / s2, cy2], [0, 0, 1]])
    return R.unit_sign((T2i @ Hn @ T1).reshape(9))


# ---- scenes ---------------------------------------------------------------------------------------------------------

def contaminated_plane(rng, members=400, contaminants=40, noise=0.5, offset=2.5):
    """`members` correspondences of one plane with `noise` px of Gaussian noise on the targets, then `contaminants` more whose
    targets lie about `offset` px to ONE side of the plane's (a fixed direction, 0.3 px of scatter), shuffled:
    (src, dst, H_true[9], on_plane[n])."""
    n = members + contaminants
    src, dst, H_true, _ = R.plane_scene(rng, n, 0.0)
    ang = rng.uniform(0, 2 * np.pi)
    side = np.array([np.cos(ang), np.sin(ang)])
    on_plane = np.zeros(n, bool)
    on_plane[rng.permutation(n)[:members]] = True
    dst = dst.copy()
    dst[on_plane] += rng.normal(0, noise, size=(members, 2))
    dst[~on_plane] += offset * side + rng.normal(0, 0.3, size=(contaminants, 2))
    return src, np.ascontiguousarray(dst), H_true, on_plane


def rms_to_truth(src, H, H_true, idx):
    """RMS distance over the points idx between where H and where H_true carry them."""
    p = np.concatenate([src[idx], np.ones((idx.size, 1))], axis=1)
    a = p @ np.asarray(H).reshape(3, 3).T
    b = p @ np.asarray(H_true).reshape(3, 3).T
    d = a[:, :2] / a[:, 2:3] - b[:, :2] / b[:, 2:3]
    return float(np.sqrt((d * d).sum(axis=1).mean()))
