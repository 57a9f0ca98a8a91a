"""CPU tests of the numpy twin of the selection ranked by MSAC weight (tests/select_msac_numpy.py; include/multih_hip.h,
mh_select_greedy_msac): its loop against the oracle's sequential selection, its weight rule on hand-built sets, and the export
table of the engine and the host layer."""
import ctypes as C
import os

import numpy as np
import pytest

import select_msac_numpy as T

THR2 = 2.2 ** 2


@pytest.fixture(scope="module")
def scene(synth, oracle):
    sc = synth.make_scene(1500, 3, seed=9, with_neighbours=False)
    with np.errstate(all="ignore"):
        H, _, _ = oracle.dlt4(sc.src, sc.dst, oracle.sample4(21, 0, 1200, sc.n))
    return sc, H


@pytest.mark.parametrize("holes", [False, True])
def test_ranked_by_count_the_twin_is_the_oracle(scene, oracle, holes):
    sc, H = scene
    mask = np.ones(sc.n, np.uint8)
    if holes:
        mask[::5] = 0
    with np.errstate(all="ignore"):
        H_o, idx_o, cnt_o, mask_o = oracle.select_greedy(sc.src, sc.dst, H, THR2, 20, 8, mask)
    H_t, idx_t, cnt_t, _, mask_t = T.select_greedy(sc.src, sc.dst, H, THR2, 20, 8, mask, rank_by="count")
    assert len(idx_o) >= 3
    assert np.array_equal(idx_t, idx_o) and np.array_equal(cnt_t, cnt_o) and np.array_equal(mask_t, mask_o)
    assert np.array_equal(H_t.view(np.uint64), H_o.view(np.uint64))
    assert np.array_equal(H_t.view(np.uint64), H[idx_t].view(np.uint64))


def test_ranked_by_count_with_the_refit_the_twin_is_the_oracle(scene, oracle):
    sc, H = scene
    with np.errstate(all="ignore"):
        H_o, idx_o, cnt_o, mask_o = oracle.select_greedy_refit(sc.src, sc.dst, sc.aff, sc.F, sc.e2, H, THR2, 20, 8)
    H_t, idx_t, cnt_t, _, mask_t = T.select_greedy(sc.src, sc.dst, H, THR2, 20, 8, rank_by="count",
                                                   refit=T.haf_refit(sc.src, sc.dst, sc.aff, sc.F, sc.e2))
    assert len(idx_o) >= 3 and not np.array_equal(H_o, H[idx_o])
    assert np.array_equal(idx_t, idx_o) and np.array_equal(cnt_t, cnt_o) and np.array_equal(mask_t, mask_o)
    assert np.array_equal(H_t.view(np.uint64), H_o.view(np.uint64))


def test_ranked_by_weight_on_a_scene(scene):
    """Weights fall from round to round, every winner is eligible, counts and weights are those of the winner on the support set
    it was selected on."""
    import msac_numpy as W
    sc, H = scene
    H_t, idx, cnt, wgt, mask = T.select_greedy(sc.src, sc.dst, H, THR2, 20, 8)
    assert len(idx) >= 3 and (cnt >= 20).all() and len(set(idx.tolist())) == len(idx)
    S = np.ones(sc.n, np.uint8)
    for k in range(len(idx)):
        c, w = W.score_msac(sc.src, sc.dst, H, THR2, S)
        ok = c >= 20
        assert w[idx[k]] == wgt[k] == w[ok].max() and c[idx[k]] == cnt[k]
        assert idx[k] == np.flatnonzero(ok & (w == wgt[k]))[0]
        with np.errstate(all="ignore"):
            S[W.pair_terms(T.O.residual_matrix(sc.src, sc.dst, H[idx[k]])[0], THR2)[0]] = 0
    assert np.array_equal(S, mask)


def test_the_tight_model_beats_the_sloppy_one_by_weight_only():
    src, dst, H = T.tight_and_sloppy(THR2)
    by_c = T.select_greedy(src, dst, H, THR2, 20, 8, rank_by="count")
    by_w = T.select_greedy(src, dst, H, THR2, 20, 8)
    assert by_c[1].tolist() == [0, 1] and by_c[2].tolist() == [40, 30]
    assert by_w[1].tolist() == [1, 0] and by_w[2].tolist() == [30, 40] and by_w[3][0] == 30 * 256
    assert 40 * 48 <= by_w[3][1] <= 40 * 50                         # about 49 each
    assert by_w[4].sum() == 0
    # need = 35: the tight model is not eligible, whatever its weight
    for rank_by in ("count", "weight"):
        r = T.select_greedy(src, dst, H, THR2, 35, 8, rank_by=rank_by)
        assert r[1].tolist() == [0] and r[2].tolist() == [40] and r[4].sum() == 30


def test_ties_go_to_the_lowest_position():
    src, dst, H = T.tie(THR2)
    _, idx, cnt, wgt, mask = T.select_greedy(src, dst, H, THR2, 20, 8)
    assert idx.tolist() == [3] and cnt.tolist() == [40] and 0 < wgt[0] < 40 * 256 and mask.sum() == 0


def test_an_eligible_candidate_of_weight_zero_wins():
    src, dst, H = T.weight_zero(THR2)
    _, idx, cnt, wgt, mask = T.select_greedy(src, dst, H, THR2, 20, 8)
    assert idx.tolist() == [1] and cnt.tolist() == [25] and wgt.tolist() == [0] and mask.sum() == 0
    assert len(T.select_greedy(src, dst, H, THR2, 26, 8)[1]) == 0


def test_a_finite_but_lighter_refit_is_not_taken(mh):
    """The sub-case of the GPU refit test, built here first: the refit keeps the hypothesis' count and weighs less."""
    sc, H, e2 = T.lighter_refit_scene(mh.synth)
    refit = T.haf_refit(sc.src, sc.dst, sc.aff, sc.F, e2)
    H_w, idx_w, cnt_w, wgt_w, _ = T.select_greedy(sc.src, sc.dst, H, THR2, 20, 8, refit=refit)
    H_c, idx_c, cnt_c, _, _ = T.select_greedy(sc.src, sc.dst, H, THR2, 20, 8, rank_by="count", refit=refit)
    assert len(idx_w) >= 2 and idx_w[0] in (0, 1) and wgt_w[0] == 256 * cnt_w[0]
    assert np.array_equal(H_w[0], H[idx_w[0]]), "by weight the hypothesis stays"
    hr = refit(H[idx_w[0]].copy(), np.ones(sc.n, bool) & (T.O.residual_matrix(sc.src, sc.dst, H[idx_w[0]])[0] < THR2))
    assert np.isfinite(hr).all()
    c, w = T.W.score_msac(sc.src, sc.dst, hr, THR2)
    assert c[0] == cnt_w[0] and w[0] < wgt_w[0]
    assert idx_c[0] == np.argmax(T.W.score_msac(sc.src, sc.dst, H, THR2)[0]) and np.array_equal(H_c[0], refit(H[idx_c[0]].copy(), T.O.residual_matrix(sc.src, sc.dst, H[idx_c[0]])[0] < THR2)), "by count the refit is taken"


def test_the_entry_point_and_the_hook_are_exported(mh, engine_lib):
    assert "mh_select_greedy_msac" in mh.capi.SYMBOLS
    # refused before any device work: a null engine
    assert engine_lib.mh_select_greedy_msac(None, C.c_double(THR2), 20, 8, None, None, None, None, None, None, C.c_longlong(0)) == -2
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    assert hasattr(host, "mhh_set_selection_score")
