"""mh_polish_homographies (include/multih_hip.h; csrc/polish_h.hip, k_polish_h) in numpy: the TWIN of the rule in the header,
operation for operation, so that the kernel can be held to it bit for bit.

    compute        OpenCV's HomographyRefineCallback as the header states it, vectorised over the members (numpy never contracts a
                   multiplication and an addition; the division rounds correctly);
    sums           refit_h_numpy.strided_tree_sum, the engine's order (thread t of 256, then the binary tree);
    jacobi_sym     the cyclic Jacobi of csrc/mh_device.hpp (jacobi_sym_dev) restated here — not numpy.linalg.eigh, whose
                   eigenvectors differ in the last bits and in sign;
    pinv_solve /   sym_eig_solve3's cut on the eigenvalues;
    pinv_diag
    polish_one     LMSolverImpl::run (M/Utilities.hpp:762-869) for eight parameters, with the header's added stop;
    polish         the call: one model per label.

tests/test_polish_h_cpu.py holds the twin to scipy's least-squares optimum; tests/test_gpu_polish_h.py holds the kernel to the
twin.  `trace` (a list) receives, per iteration, (lambda before the solve, R, accepted, took the lambda == 0 branch, dropped
eigenvalues)."""
import numpy as np

from refit_h_numpy import strided_tree_sum

MAX_ITERATIONS = 32
DEPS = 2.220446049250313e-16
FEPS = 1.1920928955078125e-07
F = np.float64


def jacobi_sym(a_in):
    """jacobi_sym_dev(n): (d[n], V[n, n] with the eigenvectors as columns).  Sweeps p < q in lexicographic order, exact-zero
    off-diagonals skipped, stop at off^2 <= 1e-30 diag^2 or after 30 sweeps."""
    a = np.array(a_in, dtype=np.float64)
    n = a.shape[0]
    v = np.eye(n)
    with np.errstate(all="ignore"):
        for _ in range(30):
            off, diag = F(0.0), F(0.0)
            for i in range(n):
                diag = diag + a[i, i] * a[i, i]
                for j in range(i + 1, n):
                    off = off + a[i, j] * a[i, j]
            if off <= F(1e-30) * diag:
                break
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = a[p, q]
                    if apq == 0.0:
                        continue
                    theta = (a[q, q] - a[p, p]) / (F(2.0) * apq)
                    sg = F(1.0) if theta >= 0.0 else F(-1.0)
                    t = sg / (np.abs(theta) + np.sqrt(theta * theta + F(1.0)))
                    c = F(1.0) / np.sqrt(t * t + F(1.0))
                    s = t * c
                    akp, akq = a[:, p].copy(), a[:, q].copy()             # (row k touches its own two entries only)
                    a[:, p] = c * akp - s * akq
                    a[:, q] = s * akp + c * akq
                    apk, aqk = a[p, :].copy(), a[q, :].copy()
                    a[p, :] = c * apk - s * aqk
                    a[q, :] = s * apk + c * aqk
                    vkp, vkq = v[:, p].copy(), v[:, q].copy()
                    v[:, p] = c * vkp - s * vkq
                    v[:, q] = s * vkp + c * vkq
    return np.diagonal(a).copy(), v


def _eig_kept(M):
    w, V = jacobi_sym(M)
    cut = F(0.0)
    for k in range(w.size):
        cut = cut + np.abs(w[k])
    cut = cut * F(2.0 * DEPS)
    kept = [k for k in range(w.size) if not (np.abs(w[k]) <= cut)]
    return w, V, kept


def pinv_solve(M, b, dropped=None):
    """pinv(M) b of the header."""
    w, V, kept = _eig_kept(M)
    n = w.size
    if dropped is not None:
        dropped.append(n - len(kept))
    out = np.zeros(n)
    with np.errstate(all="ignore"):
        for k in kept:
            proj = F(0.0)
            for i in range(n):
                proj = proj + V[i, k] * b[i]
            proj = proj / w[k]
            for i in range(n):
                out[i] = out[i] + proj * V[i, k]
    return out


def pinv_diag(M):
    """The diagonal of pinv(M) of the header."""
    w, V, kept = _eig_kept(M)
    n = w.size
    out = np.zeros(n)
    with np.errstate(all="ignore"):
        for k in kept:
            for i in range(n):
                out[i] = out[i] + V[i, k] * V[i, k] / w[k]
    return out


def residuals(src, dst, idx, x):
    """compute(x) without the Jacobian: (ww, xi, yi, rx, ry) per member."""
    X, Y, u, v = src[idx, 0], src[idx, 1], dst[idx, 0], dst[idx, 1]
    with np.errstate(all="ignore"):
        ww = (x[6] * X + x[7] * Y) + 1.0
        ww = np.where(np.abs(ww) > DEPS, 1.0 / ww, 0.0)
        xi = ((x[0] * X + x[1] * Y) + x[2]) * ww
        yi = ((x[3] * X + x[4] * Y) + x[5]) * ww
        return ww, xi, yi, xi - u, yi - v


def candidate(src, dst, idx, x):
    """Sd of a candidate: the sum S alone."""
    _, _, _, rx, ry = residuals(src, dst, idx, x)
    with np.errstate(all="ignore"):
        return strided_tree_sum(idx, (rx * rx + ry * ry).reshape(-1, 1))[0]


def compute(src, dst, idx, x):
    """compute(x) of the header: (S, A[8, 8], v[8], max |r|) from the 30 sums."""
    X, Y = src[idx, 0], src[idx, 1]
    ww, xi, yi, rx, ry = residuals(src, dst, idx, x)
    with np.errstate(all="ignore"):
        a = [X * ww, Y * ww, ww]
        bx = [-(a[0] * xi), -(a[1] * xi)]
        by = [-(a[0] * yi), -(a[1] * yi)]
        terms = [rx * rx + ry * ry]
        terms += [a[i] * rx for i in range(3)] + [a[i] * ry for i in range(3)]
        terms += [bx[0] * rx + by[0] * ry, bx[1] * rx + by[1] * ry]
        terms += [a[i] * a[j] for i in range(3) for j in range(i, 3)]
        terms += [a[i] * bx[j] for i in range(3) for j in range(2)]
        terms += [a[i] * by[j] for i in range(3) for j in range(2)]
        terms += [bx[0] * bx[0] + by[0] * by[0], bx[0] * bx[1] + by[0] * by[1], bx[1] * bx[1] + by[1] * by[1]]
        G = strided_tree_sum(idx, np.stack(terms, axis=1))
        mr = 0.0
        for val in np.concatenate([np.abs(rx), np.abs(ry)]):
            if val > mr:                                                     # (a NaN is never the largest)
                mr = val
    A = np.zeros((8, 8))
    q = 9
    for i in range(3):
        for j in range(i, 3):
            A[i, j] = A[j, i] = A[3 + i, 3 + j] = A[3 + j, 3 + i] = G[q]
            q += 1
    for i in range(3):
        for j in range(2):
            A[i, 6 + j] = A[6 + j, i] = G[15 + 2 * i + j]
            A[3 + i, 6 + j] = A[6 + j, 3 + i] = G[21 + 2 * i + j]
    A[6, 6], A[6, 7], A[7, 6], A[7, 7] = G[27], G[28], G[28], G[29]
    return G[0], A, G[1:9].copy(), mr


def polish_one(src, dst, idx, H_in, max_iterations, trace=None):
    """One model over the members idx (ascending point indices): (H_out[9], (S before, S after), (members, iterations,
    accepted, status))."""
    assert 0 <= max_iterations <= MAX_ITERATIONS
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    H_in = np.array(H_in, dtype=np.float64).reshape(9)
    with np.errstate(all="ignore"):
        x = H_in[:8] / H_in[8]
    if idx.size < 4:
        return H_in.copy(), (0.0, 0.0), (int(idx.size), 0, 0, 1)
    if not np.all(np.isfinite(x)):
        return H_in.copy(), (0.0, 0.0), (int(idx.size), 0, 0, 2)
    S, A, v, maxr = compute(src, dst, idx, x)
    S0 = S
    it = accepted = 0
    if max_iterations > 0:
        D = np.diagonal(A).copy()
        lam, lc = F(1.0), F(0.75)
        with np.errstate(all="ignore"):
            while True:
                Ap = A.copy()
                for i in range(8):
                    Ap[i, i] = A[i, i] + lam * D[i]
                dropped = []
                d = pinv_solve(Ap, v, dropped)
                xd = x - d
                Sd = candidate(src, dst, idx, xd)
                temp = np.empty(8)
                for i in range(8):
                    s = F(0.0)
                    for j in range(8):
                        s = s + A[i, j] * d[j]
                    temp[i] = -s + F(2.0) * v[i]
                dS = F(0.0)
                for i in range(8):
                    dS = dS + d[i] * temp[i]
                R = (S - Sd) / (dS if np.abs(dS) > DEPS else F(1.0))
                lam_before, zero_branch = lam, False
                if R > 0.75:
                    lam = lam * F(0.5)
                    if lam < lc:
                        lam = F(0.0)
                elif R < 0.25:
                    tt = F(0.0)
                    for i in range(8):
                        tt = tt + d[i] * v[i]
                    nu = (Sd - S) / (tt if np.abs(tt) > DEPS else F(1.0)) + F(2.0)
                    nu = F(2.0) if nu < 2.0 else nu
                    nu = F(10.0) if nu > 10.0 else nu
                    if lam == 0.0:
                        zero_branch = True
                        pd = pinv_diag(A)
                        maxval = F(DEPS)
                        for i in range(8):
                            if np.abs(pd[i]) > maxval:
                                maxval = np.abs(pd[i])
                        lam = lc = F(1.0) / maxval
                        nu = nu * F(0.5)
                    lam = lam * nu
                accept = bool(Sd < S)
                if accept:
                    S, x = Sd, xd
                    accepted += 1
                it += 1
                if trace is not None:
                    trace.append((float(lam_before), float(R), accept, zero_branch, dropped[0]))
                maxd = 0.0
                for i in range(8):
                    if np.abs(d[i]) > maxd:
                        maxd = np.abs(d[i])
                if it >= max_iterations or maxd < FEPS or not np.all(np.isfinite(d)):
                    break
                if accept:
                    _, A, v, maxr = compute(src, dst, idx, x)
                if maxr < FEPS:
                    break
    H_out = np.concatenate([x, [1.0]]) if accepted > 0 else H_in.copy()
    return H_out, (float(S0), float(S)), (int(idx.size), it, accepted, 0)


def polish(src, dst, labels, H_in, max_iterations, traces=None):
    """The twin of mh_polish_homographies: (H_out[m, 9], cost[m, 2], info int32[m, 4])."""
    labels = np.asarray(labels).reshape(-1)
    H_in = np.ascontiguousarray(H_in, np.float64).reshape(-1, 9)
    m = H_in.shape[0]
    H_out, cost, info = np.empty((m, 9)), np.empty((m, 2)), np.empty((m, 4), np.int32)
    for k in range(m):
        tr = [] if traces is not None else None
        H_out[k], cost[k], info[k] = polish_one(src, dst, np.flatnonzero(labels == k), H_in[k], max_iterations, tr)
        if traces is not None:
            traces.append(tr)
    return H_out, cost, info


def transfer_error_sum(src, dst, idx, H):
    """The sum of squared forward transfer errors of H over the members, in plain numpy (no prescribed order): for the properties."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    H = np.asarray(H, np.float64).reshape(3, 3)
    q = np.concatenate([src[idx], np.ones((len(idx), 1))], axis=1) @ H.T
    return float((((q[:, :2] / q[:, 2:3]) - dst[idx]) ** 2).sum())
