"""A numpy twin of the engine's distance-weighted smoothness (include/multih_hip.h, mh_set_smoothness_weights, MH_SMOOTH_CAUCHY;
csrc/graph.hip, k_arc_weights), written from the header's definition and sharing no code with the kernel:

    d   float32 squared distance of the arc's two sites in (x1,y1,x2,y2): coordinates cast to float32, differences, squares and the
        three additions ((dx*dx + dy*dy) + dz*dz) + dw*dw each rounded once in float32
    t   float64: r2 / (r2 + d) with r2 = rho * rho
    qf  float64: q_max * t
    q   qf >= 1.0 ? round(qf) : 1, halves away from zero (C round(); an infinite d gives t = 0, a NaN d fails the comparison)
    w   mult * q in exact integers

and a helper that writes a weighted symmetric graph as a DIRECTED hit list, every undirected pair once and repeated w times,
which is what the oracle and the reference's GCO take (a hit repeated w times is an arc of weight w: SURVEY A-2).
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

UNIFORM, CAUCHY = 0, 1                 # MH_SMOOTH_UNIFORM, MH_SMOOTH_CAUCHY
Q_MAX_LIMIT = 256                      # MH_SMOOTH_Q_MAX


def distance32(src, dst, a, b):
    """float32 squared distance of sites a[k] and b[k] in (x1,y1,x2,y2), in k_hits_filter's order of operations.  numpy rounds
    every float32 operation once and fuses nothing."""
    pv = np.concatenate([np.asarray(src, np.float64).reshape(-1, 2), np.asarray(dst, np.float64).reshape(-1, 2)], axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        pv = pv.astype(np.float32)
        diff = pv[np.asarray(a, np.int64)] - pv[np.asarray(b, np.int64)]
        sq = diff * diff
        return ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]


def quotient(d, rho, q_max):
    """q of float32 squared distances d (int64, in 1..q_max)."""
    assert 1 <= int(q_max) <= Q_MAX_LIMIT and np.isfinite(rho) and rho > 0
    d = np.asarray(d, dtype=np.float32)
    r2 = np.float64(rho) * np.float64(rho)
    with np.errstate(invalid="ignore", over="ignore"):
        qf = np.float64(q_max) * (r2 / (r2 + d.astype(np.float64)))
        ok = qf >= 1.0                                  # False for NaN
        safe = np.where(ok, qf, 1.0)
    fl = np.floor(safe)                                 # round half away from zero for safe >= 1: safe - fl is exact
    q = fl + ((safe - fl) >= 0.5)
    return np.where(ok, q, 1.0).astype(np.int64)


def arc_weights(src, dst, rowptr, col, mult, rule, rho=0.0, q_max=1):
    """The weights in force of the symmetric CSR (rowptr, col, mult): int64, one per arc."""
    mult = np.asarray(mult, dtype=np.int64)
    if rule == UNIFORM:
        return mult.copy()
    assert rule == CAUCHY
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rowptr, np.int64)))
    return mult * quotient(distance32(src, dst, rows, col), rho, q_max)


def row_sums(rowptr, w):
    """Per-site totals of the weights (int64): what the dominance pre-solve reads."""
    c = np.concatenate([[0], np.cumsum(np.asarray(w, np.int64))])
    rp = np.asarray(rowptr, np.int64)
    return c[rp[1:]] - c[rp[:-1]]


def weighted_hits(rowptr, col, w):
    """The weighted symmetric CSR as a directed hit CSR (rowptr, col int32): the pair (i, j), i < j, listed w times in row i and
    not at all in row j.  Folded back (oracle.build_sym_graph, mh_set_neighbors_csr) it is the same structure with weights w."""
    n = len(rowptr) - 1
    rp = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    w = np.asarray(w, np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    up = rows < col
    assert (w >= 1).all() and (rows != col).all()
    hr, hc = np.repeat(rows[up], w[up]), np.repeat(col[up], w[up])
    out_rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(hr, minlength=n), out=out_rp[1:])
    assert out_rp[n] <= 0x7fffffff
    return out_rp.astype(np.int32), hc.astype(np.int32)            # rows ascending already: CSR order


def knn_hits(src, dst, k):
    """Exact float32 k-NN hit lists (rowptr, col) with the engine's order of operations and tie rule (d, j)."""
    pv = np.concatenate([np.asarray(src, np.float64), np.asarray(dst, np.float64)], axis=1).astype(np.float32)
    n = pv.shape[0]
    diff = pv[:, None, :] - pv[None, :, :]
    sq = diff * diff
    d = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
    np.fill_diagonal(d, np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(n), d.shape), d), axis=1)[:, :k]
    return (np.arange(n + 1, dtype=np.int32) * k), order.reshape(-1).astype(np.int32)


def two_planes(n, seed, outliers=0.15):
    """n correspondences: two planes side by side in the first image, each moved by its own homography, plus outliers; and 4
    models (the two true ones, two near copies), i.e. 5 labels.  Returns (src, dst, H [4, 9])."""
    rng = np.random.default_rng(seed)
    src = np.stack([rng.uniform(0, 400, n), rng.uniform(0, 300, n)], axis=1)
    Ha = np.array([[1.02, 0.01, 5.0], [-0.01, 0.99, 3.0], [1e-5, 2e-5, 1.0]])
    Hb = np.array([[0.97, -0.03, 14.0], [0.02, 1.03, -6.0], [-2e-5, 1e-5, 1.0]])
    side = src[:, 0] > 200
    p = np.concatenate([src, np.ones((n, 1))], axis=1)
    qa, qb = p @ Ha.T, p @ Hb.T
    dst = np.where(side[:, None], qb[:, :2] / qb[:, 2:3], qa[:, :2] / qa[:, 2:3]) + rng.normal(0, 0.6, size=(n, 2))
    out = rng.random(n) < outliers
    dst[out] = np.stack([rng.uniform(0, 400, int(out.sum())), rng.uniform(0, 300, int(out.sum()))], axis=1)
    H = np.stack([Ha.reshape(9), Hb.reshape(9), (Ha * (1 + 2e-4 * rng.normal(size=(3, 3)))).reshape(9),
                  (Hb * (1 + 2e-4 * rng.normal(size=(3, 3)))).reshape(9)])
    return np.ascontiguousarray(src), np.ascontiguousarray(dst), np.ascontiguousarray(H)
