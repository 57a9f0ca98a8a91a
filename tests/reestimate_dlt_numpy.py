"""The per-label N-point DLT estimator (mh_set_estimator(MH_ESTIMATOR_DLT); csrc/reestimate_dlt.hip, k_dlt_reestimate) and what
the route without epipolar geometry adds on the host, in numpy.

    reestimate        H[k] = refit_h_numpy.fit over the members of label k (the header's fit(S), the kernel's TWIN bit for bit);
                      a label whose fit fails keeps its H
    dlt_refit         the refit callable of mh_set_tuning key 30 under that estimator, for select_msac_numpy.select_greedy
    select_greedy     the greedy selections with such refits: counts with oracle_lib.residual_matrix, the first maximum, the
                      winner's inliers on the support set refitted by the twin, kept when finite and not fewer (not lighter),
                      strict claim
    medoid_candidates the candidate rule of multih::MergeCandidatesMedoid (host/merge_step.cpp) on given features, modes and members
    three_motions     the scene of the tests: three independently moving planes, which no single fundamental matrix describes
"""
import types

import numpy as np

import refit_h_numpy as R
import select_msac_numpy as T

IMG = 1000.0


def reestimate(src, dst, labels, H_in):
    """(H [Nh, 9], counts [Nh]): per label refit_h_numpy.fit over np.flatnonzero(labels == k), keeping H on failure.
    Labels of -1 or >= Nh belong to nobody."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    labels = np.asarray(labels)
    H = np.array(H_in, dtype=np.float64).reshape(-1, 9)
    counts = np.zeros(H.shape[0], dtype=np.int32)
    for k in range(H.shape[0]):
        idx = np.flatnonzero(labels == k)
        counts[k] = idx.size
        h = R.fit(src, dst, idx)
        if h is not None:
            H[k] = h
    return H, counts


def dlt_refit(src, dst):
    """refit(h, own): the twin's fit over the winner's inliers `own` (flags over all points); h itself when the fit fails."""
    def refit(h, own):
        got = R.fit(src, dst, np.flatnonzero(own))
        return h if got is None else got
    return refit


def select_greedy(src, dst, H, thr2, need, max_models, mask=None, rank_by="count"):
    """mh_select_greedy (rank_by "count") / mh_select_greedy_msac ("weight") with key 30 under MH_ESTIMATOR_DLT:
    (H_selected, positions, counts, weights, mask_out)."""
    return T.select_greedy(src, dst, H, thr2, need, max_models, mask=mask, rank_by=rank_by, refit=dlt_refit(src, dst))


def features(H):
    """The 6-D merge features (M/MultiH.cpp:364-390): the images of (0,0), (1,0), (0,1)."""
    h = np.asarray(H, np.float64).reshape(-1, 9)
    return np.stack([h[:, 2] / h[:, 8], h[:, 5] / h[:, 8], (h[:, 0] + h[:, 2]) / (h[:, 6] + h[:, 8]),
                     (h[:, 3] + h[:, 5]) / (h[:, 6] + h[:, 8]), (h[:, 1] + h[:, 2]) / (h[:, 7] + h[:, 8]),
                     (h[:, 4] + h[:, 5]) / (h[:, 7] + h[:, 8])], axis=1)


def medoid_candidates(H, feat, modes, members):
    """Per mode c with members (any order): the member j with the smallest sum_k |feat[j][k] - modes[c][k]|, k = 0..5 summed
    from 0.0, the lowest j on ties; a distance that is not a number loses to one that is.  Returns (cand [nc, 9],
    cand_mode [nc]); a mode without members gives no candidate."""
    H = np.asarray(H, np.float64).reshape(-1, 9)
    cand, cand_mode = [], []
    for c, mem in enumerate(members):
        best, best_d = -1, 0.0
        for j in sorted(int(m) for m in mem):
            d = 0.0
            for k in range(6):
                d = d + abs(float(feat[j][k]) - float(modes[c][k]))
            if best < 0 or d < best_d or (best_d != best_d and d == d):          # a NaN distance never beats a number
                best, best_d = j, d
        if best >= 0:
            cand.append(H[best].copy())
            cand_mode.append(c)
    return np.array(cand).reshape(-1, 9), np.array(cand_mode, dtype=np.int32)


# ---- the three-motion scene ---------------------------------------------------------------------------------------------

def _draw_h(rng):
    """One homography drawn like refit_h_numpy.plane_scene's."""
    H = np.eye(3) + rng.normal(0, 0.08, size=(3, 3))
    H[:2, 2] = rng.uniform(-40, 40, size=2)
    H[2, :2] = rng.normal(0, 5e-5, size=2)
    H[2, 2] = 1.0
    return H


def _apply(H, pts):
    q = np.concatenate([pts, np.ones((pts.shape[0], 1))], axis=1) @ np.asarray(H).reshape(3, 3).T
    return q[:, :2] / q[:, 2:3]


def _strip(x):
    return np.minimum((np.asarray(x) * (3.0 / IMG)).astype(np.int64), 2)


def separated(Hs, sep=13.0, feat_sep=15.0):
    """synth._separated_planes' two conditions for the three strips, on a 41 x 41 grid: every strip's points are carried at
    least `sep` px apart by any other strip's H, and the merge features of any two differ by at least `feat_sep` in L1."""
    g = np.stack(np.meshgrid(np.linspace(0.0, IMG, 41), np.linspace(0.0, IMG, 41)), -1).reshape(-1, 2)
    reg = _strip(g[:, 0])
    f = features(np.array([np.asarray(h).reshape(9) for h in Hs]))
    for k in range(3):
        p = g[reg == k]
        own = _apply(Hs[k], p)
        for j in range(3):
            if j == k:
                continue
            if np.linalg.norm(_apply(Hs[j], p) - own, axis=1).min() < sep:
                return False
            if np.abs(f[j] - f[k]).sum() < feat_sep:
                return False
    return True


def three_motions(n, seed=3, noise=0.5, outlier_frac=0.25, knn=16):
    """Three vertical strips of a 1000 x 1000 image, each moving by a homography of its own (redrawn, deterministically in the
    rng, until `separated` holds), `noise` px of Gaussian noise on the targets, `outlier_frac` uniform outliers, the exact
    `knn` nearest neighbours in (x1, y1, x2, y2) as hits.  No fundamental matrix describes the pair.  Returns a namespace with
    src, dst, aff (the homographies' Jacobians; outliers near the identity), gt_label, H_true [3, 9] (unit norm, h33 >= 0),
    hit_rowptr, hit_col, n."""
    import importlib
    synth = importlib.import_module("multi-h_amd").synth
    rng = np.random.default_rng(seed)
    for _ in range(1000):
        Hs = [_draw_h(rng) for _ in range(3)]
        if separated(Hs):
            break
    else:
        raise RuntimeError("three_motions: no separated set of homographies found")
    src = rng.uniform(0.0, IMG, size=(n, 2))
    gt = _strip(src[:, 0]).astype(np.int32)
    dst = np.empty_like(src)
    aff = np.empty((n, 4))
    for k in range(3):
        m = gt == k
        dst[m] = _apply(Hs[k], src[m])
        aff[m] = synth.jacobian_h(Hs[k].reshape(9), src[m])
    dst += rng.normal(0.0, noise, size=dst.shape)
    out = rng.random(n) < outlier_frac
    dst[out] = rng.uniform(0.0, IMG, size=(int(out.sum()), 2))
    aff[out] = np.array([1.0, 0.0, 0.0, 1.0]) + rng.normal(0.0, 0.2, size=(int(out.sum()), 4))
    gt[out] = -1
    rowptr, col = synth.knn_hits(src, dst, knn, True)
    return types.SimpleNamespace(src=np.ascontiguousarray(src), dst=np.ascontiguousarray(dst), aff=np.ascontiguousarray(aff),
                                 gt_label=gt, H_true=np.array([R.unit_sign(h.reshape(9)) for h in Hs]),
                                 hit_rowptr=rowptr, hit_col=col, n=n)
