"""mh_best_alternative and mh_drop_deltas (include/multih_hip.h; csrc/label_cost.hip) in numpy, and the host's rule for the
label cost (host/merge_step.cpp: SelectMergesWithLabelCost, SelectDrop, ApplyDrop).

    cost_rows          [model, point] the engine's data term under every model, from the project's own pieces:
                       data_term_numpy.term_of_d2 on the forward error (refit_h_numpy.d2_of) or on symmetric_route_numpy.sym_d2.
    best_alternative   the TWIN of mh_best_alternative: per site the first minimum over ({-1} u U) \\ {own label} in the order
                       -1, 0, 1, ...; (alt, alt_cost, own_cost).
    drop_delta         the TWIN of one candidate of mh_drop_deltas: the members' costs, and over the symmetric graph's arcs the
                       pairs with an end in S_k, each once.
    The contract of the header — the labeling with alt in place of k costs merge_energy_numpy.labeling_energy exactly delta more
    — is a statement about drop_delta and that function, which was written independently; tests/test_label_cost_cpu.py checks it.
    select_merges, select_drop, apply_drop   the rule and the bookkeeping of MultiH's step under SetLabelCost.
"""
import numpy as np

import data_term_numpy as T
import merge_energy_numpy as M
import oracle_lib as O
import refit_h_numpy as R
import symmetric_route_numpy as S

OK, EMPTY = 0, 1
NO_DELTA = 2 ** 63 - 1                                   # LLONG_MAX
TILE = 64                                                # models per LDS tile of k_best_alternative


def cost_rows(src, dst, H, lam, thr2, term, symmetric):
    """int64 [model, point]: cost(i, H[m])."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    H = np.asarray(H, np.float64).reshape(-1, 9)
    if symmetric:
        d2 = S.sym_d2(src, dst, H)
    else:
        d2 = np.stack([R.d2_of(src, dst, h) for h in H]) if H.shape[0] else np.zeros((0, src.shape[0]))
    return T.term_of_d2(d2, lam, thr2, term).astype(np.int64)


def used_labels(labels, nh):
    labels = np.asarray(labels)
    return np.array([bool((labels == k).any()) for k in range(nh)], dtype=bool)


def best_alternative(src, dst, labels, H, lam, thr2, term, symmetric, table=None):
    """(alt int32, alt_cost int64, own_cost int64) per site.  table: the columns to choose among, [site, 1 + Nh] with the outlier
    first (mh_data_cost's own table, say); default: cost_rows."""
    labels = np.asarray(labels)
    nh = np.asarray(H).reshape(-1, 9).shape[0]
    n = labels.size
    outlier = T.outlier_cost(lam, thr2)
    if table is None:
        table = np.concatenate([np.full((n, 1), outlier, dtype=np.int64), cost_rows(src, dst, H, lam, thr2, term, symmetric).T], axis=1)
    table = np.asarray(table).astype(np.int64)
    assert table.shape == (n, nh + 1)
    allowed = np.concatenate([[True], used_labels(labels, nh)])[None, :].repeat(n, axis=0)
    allowed[np.arange(n), labels + 1] = False
    big = np.iinfo(np.int64).max
    masked = np.where(allowed, table, big)
    col = masked.argmin(axis=1)                          # numpy's argmin: the first minimum, i.e. the outlier, then the lowest index
    alt = (col - 1).astype(np.int32)
    alt_cost = masked[np.arange(n), col]
    empty = ~allowed.any(axis=1)
    alt[empty], alt_cost[empty] = -1, outlier
    own_cost = table[np.arange(n), labels + 1]
    return alt, alt_cost, own_cost


def drop_delta(labels, k, alt, alt_cost, own_cost, rowptr, col, w, lam):
    """(status, parts = (|S_k|, data_old, data_new, smooth_old, smooth_new) or None, delta) of dropping label k."""
    labels, alt = np.asarray(labels), np.asarray(alt)
    members = labels == k
    if not members.any():
        return EMPTY, None, NO_DELTA
    data_old = int(np.asarray(own_cost)[members].astype(np.int64).sum())
    data_new = int(np.asarray(alt_cost)[members].astype(np.int64).sum())
    after = np.where(members, alt, labels)
    p = np.repeat(np.arange(labels.size), np.diff(rowptr))
    q = np.asarray(col)
    once = (p > q) & (members[p] | members[q])           # both directions are stored: every undirected pair from its higher end
    wt = np.asarray(w).astype(np.int64)[once]
    potts = O.potts(lam)
    smooth_old = potts * int(wt[labels[p[once]] != labels[q[once]]].sum())
    smooth_new = potts * int(wt[after[p[once]] != after[q[once]]].sum())
    return OK, (int(members.sum()), data_old, data_new, smooth_old, smooth_new), data_new - data_old + smooth_new - smooth_old


def drop_deltas(src, dst, labels, H, cand, rowptr, col, w, lam, thr2, term, symmetric):
    """drop_delta for every candidate: (delta int64, parts int64 [ncand, 5] with zero rows where not OK, status int32, alt)."""
    alt, alt_cost, own_cost = best_alternative(src, dst, labels, H, lam, thr2, term, symmetric)
    cand = np.asarray(cand, np.int32).reshape(-1)
    delta = np.full(cand.size, NO_DELTA, dtype=np.int64)
    parts = np.zeros((cand.size, 5), dtype=np.int64)
    status = np.zeros(cand.size, dtype=np.int32)
    for c, k in enumerate(cand):
        status[c], pt, delta[c] = drop_delta(labels, int(k), alt, alt_cost, own_cost, rowptr, col, w, lam)
        if pt is not None:
            parts[c] = pt
    return delta, parts, status, alt


def labels_after_drop(labels, k, alt):
    """labels' of the header: alt in place of k, nothing renumbered."""
    return np.where(np.asarray(labels) == k, alt, labels).astype(np.int32)


def beta_of(points, lam, thr2):
    """MultiH::SetLabelCost's beta: llround(points * round(lam T))."""
    x = points * T.outlier_cost(lam, thr2)
    return int(T.c_round(x))


def select_merges(pairs, delta, status, nh, beta):
    """merge_energy_numpy.select_merges with the threshold delta - beta < 0."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    order = sorted((int(delta[k]), int(pairs[k, 0]), int(pairs[k, 1]), k) for k in range(pairs.shape[0]) if status[k] == M.OK)
    used, accepted = set(), []
    for d, a, b, k in order:
        if d - beta >= 0:
            break
        if a in used or b in used:
            continue
        used.update((a, b))
        accepted.append(k)
    return accepted


def select_drop(cand, delta, status, beta):
    """The position of the OK candidate with the smallest (delta, label) if its delta - beta < 0, else -1."""
    ok = [(int(delta[c]), int(cand[c]), c) for c in range(len(cand)) if status[c] == OK]
    if not ok:
        return -1
    d, _, c = min(ok)
    return c if d - beta < 0 else -1


def apply_drop(labels, H, k, alt):
    """(labels, H, members gone to the outlier label) after the drop of k: the members take alt, model k goes, the labels above
    k move down by one (-1 stays)."""
    H = np.array(H, dtype=np.float64).reshape(-1, 9)
    out = labels_after_drop(labels, k, alt)
    assert not (out == k).any()
    gone = int(((np.asarray(labels) == k) & (out < 0)).sum())
    out[out > k] -= 1
    return out, np.ascontiguousarray(np.delete(H, k, axis=0)), gone


def label_cost_scene(mh, patch=20):
    """The scene of the Process() test: two planes of some 600 points each among 1 600 correspondences (a quarter are outliers).
    Initial models, as in tests/test_gpu_merge_energy.py::test_process_joins_two_halves_of_a_plane: plane B's true model and, for
    plane A, two models that each fit one half of it (the true homography followed by a rotation of 0.015 rad about the centroid
    of that half's targets); and one more: the N-point refit of a patch of plane A, its `patch` members nearest to the plane's
    centroid.  Returns (scene, init models [4, 9], the patch's point indices)."""
    sc = mh.synth.make_scene(1600, 2, seed=38)
    on_a = np.flatnonzero(sc.gt_label == 0)
    centre = sc.src[on_a].mean(axis=0)
    idx = np.sort(on_a[np.argsort(((sc.src[on_a] - centre) ** 2).sum(axis=1))[:patch]])
    right = sc.src[on_a, 0] > np.median(sc.src[on_a, 0])

    def half_model(side, theta):
        c = sc.dst[side].mean(axis=0)
        ct, st = np.cos(theta), np.sin(theta)
        A = np.array([[ct, -st, c[0] - ct * c[0] + st * c[1]], [st, ct, c[1] - st * c[0] - ct * c[1]], [0.0, 0.0, 1.0]])
        Hm = A @ sc.H_true[0].reshape(3, 3)
        return (Hm / np.linalg.norm(Hm)).reshape(9)

    init = np.stack([sc.H_true[1] / np.linalg.norm(sc.H_true[1]), half_model(on_a[~right], 0.015), half_model(on_a[right], -0.015),
                     R.fit(sc.src, sc.dst, idx)])
    return sc, np.ascontiguousarray(init), idx
