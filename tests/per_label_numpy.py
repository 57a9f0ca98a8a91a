"""The per-label fits and the per-model moment sums, written from their definitions in plain numpy.

The oracle (oracle/mh_oracle.cpp) restates the engine's summation order on purpose: lane t of 256 adds the items t, t + 256,
... and a binary tree folds the lanes, so that kernel and oracle agree bit for bit.  Nothing in this file shares that order,
or any code, with either of them:

    haf_fit          GetHomographyHAFNonminimal as the header of csrc/reestimate.hip lists it: the 6 m x 4 design matrix of
                     a label's m members, A^T A accumulated in np.longdouble, numpy.linalg.eigh, H from e2, F and lambda,
                     the 1 / lambda rescale
    moments          the inlier count and the five sums per model by math.fsum (exactly rounded), the smallest eigenvalue
                     of the 3 x 3 moment matrix by eigvalsh.  The inlier decision is oracle_lib.residual_matrix(...) < thr2,
                     which is held bit-exact elsewhere: the twin is independent in the summation, not in the residual
    fit_3pt_members  oracle_lib.homography_3pt on the members, unrefined (what the 3-point tests already compare with)

and the inputs every per-label test shares: edge_labels (membership patterns at the sizes where the kernels' loops change
trips), exact_threshold_points (pairs whose forward error under the identity is exactly at, just under and just over thr2)
and same_bits (bit equality that lets NaN payloads differ).  tests/test_per_label_cpu.py holds the oracle to these
definitions; tests/test_gpu_per_label_edges.py holds the kernels to the oracle on the same inputs.
"""
import math

import numpy as np

import oracle_lib as O

LANES = 256                  # lanes of a workgroup = points of one 3-point block
HAF_TRIP = 256 * 32          # points k_haf_reestimate reads per trip of its outer loop (BATCH = 32 labels per lane)
WHOLE_BLOCK_FAR = 40         # the block pattern (h) fills when the input has it: beyond the first trip, so (e) keeps all 32 bits
EPS = 2.0 ** -52


# ---- the definitions ------------------------------------------------------------------------------------------------

def haf_rows(src, dst, aff, F, e2):
    """The six design rows per correspondence, [m, 6, 4] float64 (every entry the float64 operations of the header comment
    of csrc/reestimate.hip, left to right; numpy never contracts)."""
    src, dst, aff = np.asarray(src, np.float64), np.asarray(dst, np.float64), np.asarray(aff, np.float64)
    F = np.asarray(F, np.float64).reshape(9)
    ex, ey = float(e2[0]), float(e2[1])
    px, py, qx, qy = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
    a11, a12, a21, a22 = aff[:, 0], aff[:, 1], aff[:, 2], aff[:, 3]
    one = np.ones_like(px)
    r = np.empty((px.size, 6, 4))
    r[:, 0] = np.stack([a11 * px + qx - ex, a11 * py, a11, -F[3] * one], axis=1)
    r[:, 1] = np.stack([a12 * px, a12 * py + qx - ex, a12, -F[4] * one], axis=1)
    r[:, 2] = np.stack([a21 * px + qy - ey, a21 * py, a21, F[0] * one], axis=1)
    r[:, 3] = np.stack([a22 * px, a22 * py + qy - ey, a22, F[1] * one], axis=1)
    r[:, 4] = np.stack([ex * px - qx * px, ex * py - qx * py, ex - qx, px * F[3] + py * F[4] + F[5]], axis=1)
    r[:, 5] = np.stack([ey * px - qy * px, ey * py - qy * py, ey - qy, -(px * F[0] + py * F[1] + F[2])], axis=1)
    return r


def haf_fit(src, dst, aff, members, F, e2):
    """The HAF least-squares homography of the correspondences `members`: (H[9], the three smallest eigenvalues of A^T A in
    ascending order, |A^T A|_F).  A is 6 |members| x 4; A^T A is accumulated in np.longdouble and rounded once to float64
    for numpy.linalg.eigh."""
    members = np.asarray(members, dtype=np.int64)
    F = np.asarray(F, np.float64).reshape(9)
    ex, ey = float(e2[0]), float(e2[1])
    A = haf_rows(np.asarray(src)[members], np.asarray(dst)[members], np.asarray(aff)[members], F, e2).reshape(-1, 4)
    Al = A.astype(np.longdouble)
    AtA = (Al.T @ Al).astype(np.float64)
    w, V = np.linalg.eigh(AtA)
    h6, h7, h8, lam = V[:, 0]
    h = np.empty(9)
    h[6], h[7], h[8] = h6, h7, h8
    h[3], h[4], h[5] = ey * h6 - lam * F[0], ey * h7 - lam * F[1], ey * h8 - lam * F[2]
    h[0], h[1], h[2] = ex * h6 + lam * F[3], ex * h7 + lam * F[4], ex * h8 + lam * F[5]
    with np.errstate(all="ignore"):
        lam2 = (h[0] - ex * h[6]) / F[3]                  # the rescale RefineHomographyHAF applies in place
        H = h * (1.0 / lam2)
    return H, w[:3].copy(), float(np.linalg.norm(AtA))


def moments(src, dst, H, thr2):
    """(moments[M, 6] = n Sx Sy Sxx Sxy Syy over the inliers of each model, min_eig[M], abs_sums[M, 5] = the sums of the
    terms' magnitudes, for rounding bounds).  Every term is one float64 product, as in the kernel; the sums are exact."""
    src = np.asarray(src, np.float64)
    H = np.asarray(H, np.float64).reshape(-1, 9)
    with np.errstate(all="ignore"):
        inl = O.residual_matrix(src, dst, H) < thr2         # False for NaN
    mo = np.zeros((H.shape[0], 6))
    me = np.zeros(H.shape[0])
    mag = np.zeros((H.shape[0], 5))
    for m in range(H.shape[0]):
        x, y = src[inl[m], 0], src[inl[m], 1]
        terms = [x, y, x * x, x * y, y * y]
        mo[m, 0] = x.size
        mo[m, 1:] = [math.fsum(t) for t in terms]
        mag[m] = [math.fsum(np.abs(t)) for t in terms]
        me[m] = np.linalg.eigvalsh(moment_matrix(mo[m]))[0]
    return mo, me, mag


def moment_matrix(mo):
    """[Sxx Sxy Sx; Sxy Syy Sy; Sx Sy n] from one row n Sx Sy Sxx Sxy Syy."""
    n, sx, sy, sxx, sxy, syy = (float(v) for v in mo)
    return np.array([[sxx, sxy, sx], [sxy, syy, sy], [sx, sy, n]])


def fit_3pt_members(src, dst, members, F):
    """(H[9], finite) of the unrefined 3-point least squares over `members`."""
    m = np.asarray(members, dtype=np.int64)
    return O.homography_3pt(np.asarray(src)[m], np.asarray(dst)[m], F, refine=False)


# ---- shared inputs --------------------------------------------------------------------------------------------------

PATTERNS = "abcdefghi"


def edge_labels(n, Nh, rng, gt_label):
    """Ground-truth labels plus the membership patterns at which the per-label kernels' loops can go wrong, each on a label
    id of its own: returns (labels int32[n], where) with where[letter] = the label id, for the patterns this n and Nh have
    room for, and where["stray"] = the stray values planted.  With K = gt_label.max() + 1 ground-truth labels the ids are
    K + 0 .. K + 8 in the order of the letters; a pattern whose id is not below Nh, or whose points n does not have, is left
    out of `where` (an id left without members is one more empty label).

      a  no members
      b  1 member        c  2 members        d  3 members        (points of ground-truth label 0)
      e  one lane gets everything: every point i with i % 256 == 7 (n > 775: four members at least).  Past 8192 points
         lane 7 of k_haf_reestimate holds a full 32-bit match mask in its first trip and a remainder in its second
      f  five members in one lane's first batch, 11 + 256 * {0, 3, 4, 9, 31} (n > 7947): bit 31 of the mask is set and
         UNROLL = 4 leaves one member over
      g  members only at indices >= 8192, the second trip (n > 8192 only)
      h  a whole aligned block of 256 points, so a 3-point block rank reaches 255: block 40 where the input has one
         (then (e) skips that block's point); on a smaller input of 512 points or more block 1, less the points the
         other patterns hold there
      i  the last point n - 1 with two others from the first block (3 and 200)
      j  stray labels that belong to no model: Nh, Nh + 5, -2 and -2**31 on four points, -1 on the outliers

    The ids from K + 9 on each get 0..40 of the remaining points at random (empty, tiny and ordinary labels alike).

    The stray values are ordinary inputs, not an attempt to make a kernel fault: no kernel uses a label value as an index.
    k_haf_reestimate and the match loop of the 3-point fit only compare it for equality with their own label, and
    k_3pt_block_count and k_3pt_scatter map every value outside [0, Nh) to -1 before they use it.
    """
    gt_label = np.asarray(gt_label)
    labels = gt_label.astype(np.int32).copy()
    K = int(gt_label.max()) + 1 if n else 0
    ids = {p: K + k for k, p in enumerate(PATTERNS) if K + k < Nh}
    taken = np.zeros(n, dtype=bool)
    where = {}

    def claim(pattern, idx):
        idx = np.asarray(idx, dtype=np.int64)
        idx = idx[(idx >= 0) & (idx < n)]
        idx = idx[~taken[idx]]
        if pattern not in ids or idx.size == 0:
            return
        labels[idx] = ids[pattern]
        taken[idx] = True
        where[pattern] = ids[pattern]

    if "a" in ids:
        where["a"] = ids["a"]
    far = n >= (WHOLE_BLOCK_FAR + 1) * LANES
    if far:
        claim("h", np.arange(WHOLE_BLOCK_FAR * LANES, (WHOLE_BLOCK_FAR + 1) * LANES))
    if n >= 201:
        claim("i", [n - 1, 3, 200])
    if n > 7 + 3 * LANES:                                  # (with fewer than four members it would only repeat b, c or d)
        claim("e", np.arange(7, n, LANES))
    if n > 11 + 31 * LANES:
        claim("f", 11 + LANES * np.array([0, 3, 4, 9, 31]))
    if n > HAF_TRIP:
        tail = HAF_TRIP + np.flatnonzero(~taken[HAF_TRIP:])
        claim("g", rng.choice(tail, size=min(40, tail.size), replace=False))
    plane0 = np.flatnonzero((gt_label == 0) & ~taken)
    if plane0.size >= 6:
        take = rng.choice(plane0, size=6, replace=False)
        claim("b", take[:1])
        claim("c", take[1:3])
        claim("d", take[3:6])
    stray = [Nh, Nh + 5, -2, -2 ** 31]
    free = np.flatnonzero(~taken & (gt_label < 0))
    if free.size < len(stray):
        free = np.flatnonzero(~taken)
    spots = free[:len(stray)]
    labels[spots] = stray[:spots.size]
    taken[spots] = True
    where["stray"] = stray[:spots.size]
    if not far and n >= 2 * LANES:
        claim("h", np.arange(LANES, 2 * LANES))
    for l in range(K + len(PATTERNS), Nh):
        free = np.flatnonzero(~taken)
        k = min(int(rng.integers(0, 41)), free.size)
        if k:
            idx = rng.choice(free, size=k, replace=False)
            labels[idx] = l
            taken[idx] = True
    return labels, where


def members_of(labels, l):
    return np.flatnonzero(np.asarray(labels) == l)


def in_range_counts(labels, Nh):
    labels = np.asarray(labels)
    ok = (labels >= 0) & (labels < Nh)
    return np.bincount(labels[ok], minlength=Nh).astype(np.int32)


def exact_threshold_points(k):
    """(src[3 k, 2], dst[3 k, 2], kind[3 k]): pairs on the x axis whose forward error under the identity is exact.  For
    i = 0 .. k - 1 the source (i, 0) gets three targets: (i + 2, 0), the double next below it and the double next above it.
    The identity gives s = 1, u = i and v = 0 without rounding, and x2 - u is exact, so with thr2 = 4.0
        kind  0   d2 == 4.0 == thr2    must NOT count (the test is a strict <)
        kind -1   d2 <  4.0            must count     (for i = 0 the target is np.nextafter(2.0, 0))
        kind +1   d2 >  4.0            must not count
    The sources are exactly collinear (y = 0): the moment matrix of these inliers is singular."""
    i = np.repeat(np.arange(k, dtype=np.float64), 3)
    kind = np.tile(np.array([0, -1, 1]), k)
    x2 = i + 2.0
    x2 = np.where(kind < 0, np.nextafter(x2, -np.inf), np.where(kind > 0, np.nextafter(x2, np.inf), x2))
    z = np.zeros_like(i)
    return np.stack([i, z], axis=1), np.stack([x2, z], axis=1), kind


def same_bits(a, b):
    """True when a and b are NaN in the same places and bit-identical everywhere else (-0.0 differs from 0.0, inf from NaN)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))
