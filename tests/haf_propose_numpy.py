"""numpy twin of the HAF proposer (include/multih_hip.h, mh_propose_haf; csrc/haf_propose.hip).  Written from the definition,
out of numpy and the oracle only:

  H0             oracle.haf_point, row i (GetHomographyHAF of the anchor)
  consistency    oracle.residual_matrix(H0 as stored)[q] < thr2, strictly; a NaN is not consistent; the forward error
  the ten sums   the anchor's, then one acc = acc + s per consistent neighbour in ascending column j of row i of the table
                 (local_sampler_numpy.knn_table, its first `members` columns); every term s = r0a r0b, then s = s + rqa rqb
  the solve      oracle.jacobi_sym on the symmetric 4 x 4, the column of the smallest eigenvalue (first index on ties), rows 1-2
                 from e2, F and lambda, every entry times 1.0 / h33
  no consistent neighbour, or members == 0: the result is H0

numpy's elementwise float64 operations round once each (no fused multiply-add), which is what the definition asks for.
"""
import numpy as np

import oracle_lib as oracle
from local_sampler_numpy import knn_table      # noqa: F401  (the table of the definition; callers build it once per scene)

PAIRS = [(a, b) for a in range(4) for b in range(a, 4)]      # 00 01 02 03 11 12 13 22 23 33


def haf_rows(src, dst, aff, F, e2):
    """The six HAF rows of every correspondence: (n, 6, 4), operation for operation M/MultiH.cpp:938-966."""
    a11, a12, a21, a22 = (np.ascontiguousarray(aff[:, c], dtype=np.float64) for c in range(4))
    px, py, qx, qy = (np.ascontiguousarray(v, dtype=np.float64) for v in (src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]))
    F = np.asarray(F, dtype=np.float64).reshape(9)
    ex, ey = float(e2[0]), float(e2[1])
    n = px.size
    one = np.ones(n)
    r = np.empty((n, 6, 4))
    r[:, 0, 0] = a11 * px + qx - ex; r[:, 0, 1] = a11 * py;           r[:, 0, 2] = a11; r[:, 0, 3] = -F[3] * one
    r[:, 1, 0] = a12 * px;           r[:, 1, 1] = a12 * py + qx - ex; r[:, 1, 2] = a12; r[:, 1, 3] = -F[4] * one
    r[:, 2, 0] = a21 * px + qy - ey; r[:, 2, 1] = a21 * py;           r[:, 2, 2] = a21; r[:, 2, 3] = F[0] * one
    r[:, 3, 0] = a22 * px;           r[:, 3, 1] = a22 * py + qy - ey; r[:, 3, 2] = a22; r[:, 3, 3] = F[1] * one
    r[:, 4, 0] = ex * px - qx * px;  r[:, 4, 1] = ex * py - qx * py;  r[:, 4, 2] = ex - qx
    r[:, 4, 3] = px * F[3] + py * F[4] + F[5]
    r[:, 5, 0] = ey * px - qy * px;  r[:, 5, 1] = ey * py - qy * py;  r[:, 5, 2] = ey - qy
    r[:, 5, 3] = -(px * F[0] + py * F[1] + F[2])
    return r


def haf_terms(rows):
    """The ten A^T A terms of every correspondence: (n, 10), s = r0a r0b, then s = s + rqa rqb for q = 1 .. 5."""
    out = np.empty((rows.shape[0], 10))
    for t, (a, b) in enumerate(PAIRS):
        s = rows[:, 0, a] * rows[:, 0, b]
        for q in range(1, 6):
            s = s + rows[:, q, a] * rows[:, q, b]
        out[:, t] = s
    return out


def solve(u, F, e2):
    """Ten sums -> H (9,), the tail of GetHomographyHAF: eigen-solve, smallest eigenvalue's column, rows 1-2, 1.0 / h33."""
    F = np.asarray(F, dtype=np.float64).reshape(9)
    ex, ey = np.float64(e2[0]), np.float64(e2[1])
    a = np.empty((4, 4))
    for t, (i, j) in enumerate(PAIRS):
        a[i, j] = u[t]
        a[j, i] = u[t]
    d, v = oracle.jacobi_sym(a)
    jm = 0
    for j in range(1, 4):
        if d[j] < d[jm]:
            jm = j
    h6, h7, h8, lam = (np.float64(v[k, jm]) for k in range(4))
    h = np.empty(9)
    with np.errstate(all="ignore"):
        h[6], h[7], h[8] = h6, h7, h8
        h[3] = ey * h6 - lam * F[0]
        h[4] = ey * h7 - lam * F[1]
        h[5] = ey * h8 - lam * F[2]
        h[0] = ex * h6 + lam * F[3]
        h[1] = ex * h7 + lam * F[4]
        h[2] = ex * h8 + lam * F[5]
        inv = np.float64(1.0) / h[8]
        return h * inv


def anchors(first, m, stride):
    """Counter c = first + s, anchor i = c * stride, for s = 0 .. m - 1."""
    return (first + np.arange(m, dtype=np.int64)) * stride


def propose(src, dst, aff, F, e2, first, m, stride, members, thr2, nbr=None):
    """(H [m, 9], used [m] uint32): the batch mh_propose_haf defines.  nbr: the sampling table (needed when members > 0)."""
    src, dst, aff = (np.ascontiguousarray(v, dtype=np.float64) for v in (src, dst, aff))
    n = src.shape[0]
    idx = anchors(first, m, stride)
    assert stride >= 1 and m >= 0 and first >= 0 and (m == 0 or idx[-1] < n)
    assert members == 0 or (nbr is not None and 3 <= members <= nbr.shape[1])
    H0_all, _ = oracle.haf_point(src, dst, aff, F, e2, 0.0)
    H = H0_all[idx].copy()
    used = np.zeros(m, dtype=np.uint32)
    if members == 0 or m == 0:
        return H, used
    terms = haf_terms(haf_rows(src, dst, aff, F, e2))
    with np.errstate(all="ignore"):
        R = oracle.residual_matrix(src, dst, H)                     # row s: d2(H0 of anchor s, every point)
    for s, i in enumerate(idx):
        row = nbr[i, :members]
        ok = R[s, row] < thr2                                       # NaN < thr2 is False
        if not ok.any():
            continue
        acc = terms[i].copy()
        for j in np.nonzero(ok)[0]:
            acc = acc + terms[row[j]]
            used[s] |= np.uint32(1) << np.uint32(j)
        H[s] = solve(acc, F, e2)
    return H, used
