"""mh_merge_deltas and mh_labeling_energy (include/multih_hip.h; csrc/merge_energy.hip) in numpy, and the host's merge rule
(host/merge_step.cpp: SelectMerges, ApplyMerges).

    pair_delta        the TWIN of one pair of mh_merge_deltas, from the project's own pieces: refit_h_numpy.fit over the ascending
                      union (the engine's summation order, so H_ab can be held to it bit for bit), data_term_numpy.term_of_d2 on
                      the forward error (refit_h_numpy.d2_of) or on symmetric_route_numpy.sym_d2, and the cut over the symmetric
                      graph's arcs to a lower index.
    labeling_energy   the energy of a labeling, written INDEPENDENTLY of pair_delta: a plain loop over the sites and over the
                      undirected neighbour pairs.  The contract of the header — relabelling b -> a with H_ab as model a changes
                      the energy by exactly delta — is a statement about these two, and tests/test_merge_energy_cpu.py checks it.
    select_merges, apply_merges   the rule and the bookkeeping of MultiH's MERGE_ENERGY step.
"""
import numpy as np

import data_term_numpy as T
import oracle_lib as O
import refit_h_numpy as R
import symmetric_route_numpy as S

OK, EMPTY, NO_FIT = 0, 1, 2
NO_DELTA = 2 ** 63 - 1                                   # LLONG_MAX


def d2_under(src, dst, H, symmetric):
    """[point] the error the route measures under one model."""
    return S.sym_d2(src, dst, H)[0] if symmetric else R.d2_of(src, dst, H)


def pair_delta(src, dst, labels, H, a, b, rowptr, col, w, lam, thr2, term, symmetric):
    """(status, H_ab or None, parts = (|S|, data_old, data_new, cut) or None, delta) of the pair (a, b), a < b."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    labels = np.asarray(labels)
    H = np.asarray(H, np.float64).reshape(-1, 9)
    in_a, in_b = labels == a, labels == b
    if not in_a.any() or not in_b.any():
        return EMPTY, None, None, NO_DELTA
    members = np.flatnonzero(in_a | in_b)                # ascending
    H_ab = R.fit(src, dst, members)
    if H_ab is None:
        return NO_FIT, None, None, NO_DELTA
    ia, ib = np.flatnonzero(in_a), np.flatnonzero(in_b)
    cost = lambda idx, h: int(T.term_of_d2(d2_under(src[idx], dst[idx], h, symmetric), lam, thr2, term).astype(np.int64).sum())
    data_old = cost(ia, H[a]) + cost(ib, H[b])
    data_new = cost(members, H_ab)
    across = 0
    for p in members:
        other = a if labels[p] == b else b
        k = np.arange(rowptr[p], rowptr[p + 1])
        q = col[k]
        hit = (q < p) & (labels[q] == other)
        across += int(w[k][hit].astype(np.int64).sum())
    cut = O.potts(lam) * across
    return OK, H_ab, (int(members.size), data_old, data_new, cut), data_new - data_old - cut


def merge_deltas(src, dst, labels, H, pairs, rowptr, col, w, lam, thr2, term, symmetric):
    """pair_delta for every pair: (H_ab [npairs, 9] with NaN rows where not OK, delta int64, parts int64 [npairs, 4] with zero rows
    where not OK, status int32)."""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    Hs = np.full((pairs.shape[0], 9), np.nan)
    delta = np.full(pairs.shape[0], NO_DELTA, dtype=np.int64)
    parts = np.zeros((pairs.shape[0], 4), dtype=np.int64)
    status = np.zeros(pairs.shape[0], dtype=np.int32)
    for k, (a, b) in enumerate(pairs):
        st, h, pt, dl = pair_delta(src, dst, labels, H, int(a), int(b), rowptr, col, w, lam, thr2, term, symmetric)
        status[k], delta[k] = st, dl
        if st == OK:
            Hs[k], parts[k] = h, pt
    return Hs, delta, parts, status


def labeling_energy(src, dst, labels, H, rowptr, col, w, lam, thr2, term, symmetric):
    """(energy, data, smooth) of labels (-1 .. Nh-1) under the models H: a loop over the sites, then over the undirected pairs."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    H = np.asarray(H, np.float64).reshape(-1, 9)
    n = src.shape[0]
    outlier = T.outlier_cost(lam, thr2)
    data = 0
    for i in range(n):
        l = int(labels[i])
        if l < 0:
            data += outlier
        else:
            d2 = d2_under(src[i:i + 1], dst[i:i + 1], H[l], symmetric)
            data += int(T.term_of_d2(d2, lam, thr2, term)[0])
    seen = {}
    for p in range(n):                                   # the multiplicity of every undirected pair {p, q}, p != q, once
        for k in range(int(rowptr[p]), int(rowptr[p + 1])):
            q = int(col[k])
            if q != p:
                key = (min(p, q), max(p, q))
                assert seen.setdefault(key, int(w[k])) == int(w[k]), "the graph is not symmetric"
    differ = sum(m for (p, q), m in seen.items() if labels[p] != labels[q])
    smooth = O.potts(lam) * differ
    return data + smooth, data, smooth


def select_merges(pairs, delta, status, nh):
    """Positions of the accepted pairs, in acceptance order: OK pairs by (delta, a, b) ascending while delta < 0, no label twice."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    order = sorted((int(delta[k]), int(pairs[k, 0]), int(pairs[k, 1]), k) for k in range(pairs.shape[0]) if status[k] == OK)
    used, accepted = set(), []
    for d, a, b, k in order:
        if d >= 0:
            break
        if a in used or b in used:
            continue
        used.update((a, b))
        accepted.append(k)
    return accepted


def apply_merges(labels, H, pairs, H_ab, accepted):
    """(labels, H) after the accepted joins: b -> a, model a = the pair's H_ab, the removed models dropped and the labels
    renumbered densely in the old order (-1 stays)."""
    labels = np.array(labels, dtype=np.int32)
    H = np.array(H, dtype=np.float64).reshape(-1, 9)
    pairs = np.asarray(pairs).reshape(-1, 2)
    gone = []
    for k in accepted:
        a, b = int(pairs[k, 0]), int(pairs[k, 1])
        labels[labels == b] = a
        H[a] = np.asarray(H_ab, np.float64).reshape(-1, 9)[k]
        gone.append(b)
    keep = np.array([l for l in range(H.shape[0]) if l not in gone], dtype=np.int64)
    new_index = np.full(H.shape[0], -1, dtype=np.int32)
    new_index[keep] = np.arange(keep.size, dtype=np.int32)
    out = labels.copy()
    out[labels >= 0] = new_index[labels[labels >= 0]]
    return out, np.ascontiguousarray(H[keep])
