"""A numpy twin of the symmetric route (include/multih_hip.h, mh_set_residual_scope(MH_RESIDUAL_SCOPE_ROUTE) under
MH_RESIDUAL_SYMMETRIC): the data term's table and the LabelingStep on the symmetric transfer error.

Almost nothing is new.  d2 is oracle_lib.residual_matrix_sym — bit-equal to the engine's symmetric residual, which
tests/test_symmetric_exact.py holds to exact rationals —, the cost of a pair is data_term_numpy.term_of_d2 on it (the header's
table, unchanged: both terms, label 0, T = thr2 * 81 / 16, C round()), and the step is data_term_numpy.labeling_step_twin with
that table in place of the forward one.
"""
import numpy as np

import data_term_numpy as T
import oracle_lib as O

REFERENCE, RISING = T.REFERENCE, T.RISING


def sym_d2(src, dst, H):
    """[model, point] symmetric transfer error; NaN / inf where the engine has them."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, 9)
    with np.errstate(all="ignore"):
        return O.residual_matrix_sym(src, dst, H)


def cost_matrix(src, dst, H, lam, thr2, term=REFERENCE):
    """The model-major matrix of mh_cost_matrix under the symmetric route: C[m, i]."""
    return T.term_of_d2(sym_d2(src, dst, H), lam, thr2, term)


def cost_table(src, dst, H, lam, thr2, term=REFERENCE):
    """The site-major table of mh_data_cost under the symmetric route: cost[i, l], label 0 the outlier, l >= 1 model l - 1."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, 9)
    cost = np.empty((np.asarray(src).shape[0], H.shape[0] + 1), dtype=np.int32)
    cost[:, 0] = T.outlier_cost(lam, thr2)
    if H.shape[0]:
        cost[:, 1:] = cost_matrix(src, dst, H, lam, thr2, term).T
    return cost


def labeling_step_twin(src, dst, aff, H, lam, thr2, rowptr, col, warm, F, e2, labeling, term=REFERENCE):
    """data_term_numpy.labeling_step_twin with the symmetric table: table -> expansion (warm start iff warm, from
    labeling + 1) -> labels - 1 -> per-label HAF re-estimation.  Returns (labels, H, energy, cycles)."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, 9)
    cost = cost_table(src, dst, H, lam, thr2, term)
    init = (np.asarray(labeling, dtype=np.int32) + 1) if warm else None
    lab, energy, cycles, _ = O.expand(cost, rowptr, col, O.potts(lam), init)
    lab = (lab - 1).astype(np.int32)
    H2, _ = O.haf_reestimate(src, dst, aff, lab, H, F, e2)
    return lab, H2, energy, cycles
