"""A numpy twin of the greedy selection ranked by MSAC weight (include/multih_hip.h, mh_select_greedy_msac).

The header's rule once more, sequentially and in float64.  Per round, on the support set S (mask != 0):

    count_c, weight_c   of every candidate over S, as msac_numpy.pair_terms defines a pair (d2 from oracle_lib.residual_matrix,
                        bit-equal to the engine's forward residual)
    eligible            count_c >= need and not selected before
    winner              rank_by = "weight": the eligible candidate of the highest weight; rank_by = "count": of the highest
                        count (the rule of mh_select_greedy, oracle/mh_oracle.cpp section 12); the lowest position on ties;
                        nobody eligible ends the selection
    refit (optional)    refit(h, own) -> 9 doubles, own = the winner's inliers on S; it takes the winner's place in the claim and
                        in H when it is finite (every |entry| < 2^1000) and its score on S — weight or count, as ranked — is at
                        least the hypothesis'
    claim               the inliers (d2 < thr2, strictly) of the model that claims leave S

tests/test_select_msac_cpu.py pins the loop to oracle_lib.select_greedy / select_greedy_refit with rank_by = "count" and the
weight rule to hand-built sets; the builders of those sets are here because the GPU tests run the same ones."""
import numpy as np

import msac_numpy as W
import oracle_lib as O


def select_greedy(src, dst, H, thr2, need, max_models, mask=None, rank_by="weight", refit=None):
    """Returns (H_selected [k, 9], positions [k], counts [k], weights [k], mask_out [n] uint8)."""
    assert rank_by in ("count", "weight")
    H = np.ascontiguousarray(H, dtype=np.float64).reshape(-1, 9)
    n = np.asarray(src).shape[0]
    with np.errstate(all="ignore"):
        d2 = O.residual_matrix(src, dst, H)                         # [candidate, point], computed once: S only shrinks
    inl, w = W.pair_terms(d2, thr2)
    S = np.ones(n, dtype=bool) if mask is None else np.asarray(mask) != 0
    taken = np.zeros(H.shape[0], dtype=bool)
    Hs, pos, cnts, wgts = [], [], [], []
    for _ in range(max_models):
        cnt = inl[:, S].sum(axis=1)
        wgt = w[:, S].sum(axis=1, dtype=np.int64)
        eligible = (cnt >= need) & ~taken
        if not eligible.any():
            break
        score = wgt if rank_by == "weight" else cnt
        bm = int(np.argmax(np.where(eligible, score, -1)))          # the first maximum: the lowest position
        taken[bm] = True
        h, claim = H[bm], inl[bm] & S
        if refit is not None:
            hr = np.asarray(refit(H[bm].copy(), claim), dtype=np.float64).reshape(9)
            if bool(np.all(np.abs(hr) < 2.0 ** 1000)):              # (False for NaN)
                with np.errstate(all="ignore"):
                    inr, wr = W.pair_terms(O.residual_matrix(src, dst, hr)[0], thr2)
                sr = int(wr[S].sum(dtype=np.int64)) if rank_by == "weight" else int(inr[S].sum())
                if sr >= int(score[bm]):
                    h, claim = hr, inr & S
        Hs.append(h.copy()); pos.append(bm); cnts.append(int(cnt[bm])); wgts.append(int(wgt[bm]))
        S = S & ~claim
    return (np.array(Hs).reshape(-1, 9), np.array(pos, dtype=np.int64), np.array(cnts, dtype=np.int32),
            np.array(wgts, dtype=np.int32), S.astype(np.uint8))


def haf_refit(src, dst, aff, F, e2):
    """The refit callable of mh_set_tuning key 30 under MH_ESTIMATOR_HAF: oracle_lib.haf_reestimate with one label."""
    def refit(h, own):
        return O.haf_reestimate(src, dst, aff, np.where(own, 0, -1).astype(np.int32), h.reshape(1, 9), F, e2)[0][0]
    return refit


# ---- hand-built sets (CPU and GPU tests) -------------------------------------------------------------------------------------
def shift(dx, dy=0.0):
    return np.array([1.0, 0.0, dx, 0.0, 1.0, dy, 0.0, 0.0, 1.0])


def tight_and_sloppy(thr2):
    """30 points exactly on H_a (a shift by 100), 40 points that fit H_b (the identity) at 0.9 of the threshold DISTANCE
    (d2 = 0.81 thr2: each weighs about 49).  Batch = [H_b, H_a]: by count H_b (40) comes first, by weight H_a (30 x 256)."""
    rng = np.random.default_rng(11)
    src = np.floor(rng.uniform(0, 500, size=(70, 2)))
    dst = src.copy()
    dst[:30, 0] += 100.0
    dst[30:, 0] += 0.9 * np.sqrt(thr2)
    return src, dst, np.array([shift(0.0), shift(100.0)])


def tie(thr2):
    """40 points on a shift by 50; the same H at positions 3 and 7 of a batch whose other models explain nothing."""
    rng = np.random.default_rng(12)
    src = np.floor(rng.uniform(0, 500, size=(40, 2)))
    dst = src + np.array([50.0, 0.0]) + rng.uniform(-0.4, 0.4, size=(40, 2)) * np.sqrt(thr2)
    H = np.array([shift(1000.0 + 10 * i) for i in range(9)])
    H[3] = H[7] = shift(50.0)
    return src, dst, H


def weight_zero(thr2):
    """25 points with dst = src and a shift whose offset makes d2 about 0.999 thr2: count 25, weight 0."""
    rng = np.random.default_rng(13)
    src = np.floor(rng.uniform(0, 500, size=(25, 2)))
    return src, src.copy(), np.array([shift(1000.0), shift(np.sqrt(0.999 * thr2))])


def lighter_refit_scene(synth_module):
    """A scene whose planes' own homographies are in the batch and fit their points exactly (no noise on the points), and an
    epipole 0.1 % off: the HAF refit of such a winner is finite and keeps every inlier, but fits worse than the hypothesis —
    ranked by weight the hypothesis is kept, ranked by count the refit is taken.  Returns (scene, batch, the epipole to set);
    the batch ends with slightly perturbed copies of the planes' models."""
    sc = synth_module.make_scene(600, 2, seed=41, outlier_frac=0.2, noise=0.0, with_neighbours=False, legacy_r04=False)
    rng = np.random.default_rng(41)
    H = np.concatenate([sc.H_true, np.tile(sc.H_true, (3, 1)) * (1.0 + rng.normal(0.0, 2e-4, size=(6, 9)))])
    return sc, np.ascontiguousarray(H), sc.e2 * 1.001
