"""A numpy twin of the engine's data term (include/multih_hip.h, mh_set_data_term) and of the steps that consume it.

The oracle's dataEnergy is the reference's and stays so; under MH_DATA_TERM_RISING there is no oracle, so the rule is
written out here once more, from the header's table, in float64:

    lam = 100 / lambda        T = thr2 * 81 / 16        B = round(lam * T)
    label 0            -> B
    d2 < T (strictly)  -> round(lam * (1.0 - (d2 / T)))   REFERENCE (0)
                          round(lam * (d2 / T))           RISING (1)
    otherwise (NaN)    -> 2 * B

d2 comes from oracle_lib.residual_matrix (bit-equal to the engine's forward residual), every numpy operation below is one
IEEE double operation (numpy never contracts), and round() is C round() spelt out — halves away from zero; np.round rounds
halves to even and is not used.  tests/test_data_term_cpu.py shows that under REFERENCE the twin IS the oracle (table,
LabelingStep, the whole loop), which is what entitles it to stand in for one under RISING.
"""
import numpy as np

import oracle_lib as O

REFERENCE, RISING = 0, 1


def c_round(x):
    """C round() for x >= 0: halves away from zero.  x - trunc(x) is exact for a double, so the comparison is too."""
    x = np.asarray(x, dtype=np.float64)
    t = np.trunc(x)
    return t + (x - t >= 0.5)


def term_of_d2(d2, lam, thr2, term):
    """The int32 cost of pairs with forward error d2 (any shape) against a model label (l >= 1)."""
    assert term in (REFERENCE, RISING)
    d2 = np.asarray(d2, dtype=np.float64)
    lam_ = 100.0 / lam
    T = thr2 * 81.0 / 16.0
    beyond = 2 * int(c_round(lam_ * T))
    with np.errstate(all="ignore"):
        q = d2 / T
        inner = (1.0 - q) if term == REFERENCE else q
        near = d2 < T                                   # False for NaN
        val = c_round(np.where(near, lam_ * inner, 0.0))
    return np.where(near, val, beyond).astype(np.int32)


def outlier_cost(lam, thr2):
    return int(c_round((100.0 / lam) * (thr2 * 81.0 / 16.0)))


def cost_table(src, dst, H, lam, thr2, term):
    """The site-major table of mh_data_cost: cost[i, l], label 0 the outlier, l >= 1 model l - 1."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, 9)
    n = np.asarray(src).shape[0]
    cost = np.empty((n, H.shape[0] + 1), dtype=np.int32)
    cost[:, 0] = outlier_cost(lam, thr2)
    if H.shape[0]:
        with np.errstate(all="ignore"):
            d2 = O.residual_matrix(src, dst, H)         # [model, point]
        cost[:, 1:] = term_of_d2(d2, lam, thr2, term).T
    return cost


def labeling_step_twin(src, dst, aff, H, lam, thr2, rowptr, col, warm, F, e2, labeling, term):
    """LabelingStep (M/MultiH.cpp:513-602) with the selected data term: table -> expansion (warm start iff warm, from
    labeling + 1) -> labels - 1 -> per-label HAF re-estimation.  Returns (labels, H, energy, cycles) as oracle_lib.labeling_step."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, 9)
    cost = cost_table(src, dst, H, lam, thr2, term)
    init = (np.asarray(labeling, dtype=np.int32) + 1) if warm else None
    lab, energy, cycles, _ = O.expand(cost, rowptr, col, O.potts(lam), init)
    lab = (lab - 1).astype(np.int32)
    H2, _ = O.haf_reestimate(src, dst, aff, lab, H, F, e2)
    return lab, H2, energy, cycles


def loop_twin(src, dst, aff, H0, F, e2, lam, thr_h, rowptr, col, seed, term, fixed_iterations=0):
    """ClusterMergingAndLabeling (M/MultiH.cpp:263-311) with the selected data term: MergingStep with the product's step
    seeds, warm start iff the merge changed nothing, the stop rule of :295, the one- and zero-cluster exits.  Returns
    (labels, H, iterations, energy) as oracle_lib.cluster_merging_and_labeling does."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    thr2 = thr_h * thr_h
    models = np.asarray(H0, dtype=np.float64).reshape(-1, 9).copy()
    n = src.shape[0]
    labeling = np.full(n, -1, dtype=np.int32)                       # :263
    last_energy, final_energy = 2147483647.0, 0.0                   # :264
    not_changed, iteration, step = 0, 0, 0
    while iteration < 500:                                          # :267
        iteration += 1
        changed = False
        if models.shape[0] > 0:
            kept, changed, _ = O.merging_step(src, dst, models, F, thr_h, seed ^ 0x4d53 ^ (step << 20))
            step += 1
            if changed:
                models = kept                                       # :469-470
        not_changed = 0 if changed else not_changed + 1             # :275-278
        if models.shape[0] == 1:                                    # :280-285
            with np.errstate(all="ignore"):
                labeling[O.residual_matrix(src, dst, models)[0] < thr2] = 0
            break
        if models.shape[0] == 0:
            break
        labeling, models, energy_i, _ = labeling_step_twin(src, dst, aff, models, lam, thr2, rowptr, col, not changed, F, e2,
                                                           labeling, term)
        energy = float(energy_i)
        if (not changed and abs(last_energy - energy) < 1e-5) or not_changed > 10 or \
                (fixed_iterations > 0 and iteration >= fixed_iterations):   # :295
            final_energy = energy
            break
        last_energy = energy
    else:
        iteration += 1          # `while (iteration++ < 500)` left by its condition: the counter was bumped once more
    return labeling, models, iteration - 1, final_energy             # :311
