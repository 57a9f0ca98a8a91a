"""A numpy twin of the MSAC-weighted score (include/multih_hip.h, mh_score_msac).

There is no oracle for the weights, so the header's rule is written out here once more, in float64:

    d2 < thr2 (strictly)   the pair counts 1 and weighs round(256.0 * (1.0 - (d2 / thr2)))
    otherwise (inf, NaN)   the pair counts 0 and weighs 0
    count[m], weight[m] =  int32 sums over the points with mask != 0

d2 comes from oracle_lib.residual_matrix (bit-equal to the engine's forward residual), every numpy operation below is one
IEEE double operation (numpy never contracts), and round() is C round() — data_term_numpy.c_round, halves away from zero;
np.round rounds halves to even and is not used.  tests/test_msac_cpu.py pins the twin's counts to oracle_lib.score and its
weights to known answers.
"""
import numpy as np

import oracle_lib as O
from data_term_numpy import c_round

SCALE = 256            # MH_MSAC_SCALE


def pair_terms(d2, thr2):
    """(counted, weight) of pairs with forward error d2 (any shape): bool and int32 arrays."""
    d2 = np.asarray(d2, dtype=np.float64)
    with np.errstate(all="ignore"):
        inl = d2 < thr2                                 # False for NaN
        q = d2 / thr2
        gain = float(SCALE) * (1.0 - q)
        w = c_round(np.where(inl, gain, 0.0))
    return inl, np.where(inl, w, 0).astype(np.int32)


def sums_of_d2(d2, thr2, mask=None):
    """(counts, weights) per model from the [model, point] matrix of forward errors."""
    inl, w = pair_terms(d2, thr2)
    if mask is not None:
        keep = np.asarray(mask) != 0
        inl, w = inl[:, keep], w[:, keep]
    return inl.sum(axis=1).astype(np.int32), w.sum(axis=1, dtype=np.int64).astype(np.int32)


def score_msac(src, dst, H, thr2, mask=None):
    """(counts, weights) of the models H (m x 9) over the correspondences, as mh_score_msac returns them."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, 9)
    with np.errstate(all="ignore"):
        d2 = O.residual_matrix(src, dst, H)             # [model, point]
    return sums_of_d2(d2, thr2, mask)


def best_by_weight(weights):
    """Index of the highest weight, the lowest index on ties (mh_select_best_msac)."""
    return int(np.argmax(np.asarray(weights)))          # np.argmax returns the first maximum
