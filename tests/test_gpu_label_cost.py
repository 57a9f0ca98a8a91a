"""mh_best_alternative and mh_drop_deltas on the GPU (csrc/label_cost.hip: k_best_alternative, k_drop_label) and the label cost of
MultiH's MERGE_ENERGY step (SetLabelCost).  Everything is integer and compared EXACTLY with the twin (tests/label_cost_numpy.py): at
the site and tile edges of the arg-min — also against the arg-min over mh_data_cost's own table —, at the member-loop edges of the
drop, on long and on irregular graph rows, under both data terms and both errors with the contract through mh_labeling_energy on
the device, at the argument and state edges, and through Process() and the harness."""
import ctypes as C
import os

import numpy as np
import pytest

import data_term_numpy as T
import label_cost_numpy as L
import merge_energy_numpy as M
import refit_h_numpy as R

pytestmark = pytest.mark.gpu

INVALID, NOT_SET = -2, -4
LAM, THR2 = 0.5, 2.2 ** 2                                 # the engine fixture's lambda and thr_hom^2
OUTLIER = T.outlier_cost(LAM, THR2)
TERMS = {T.REFERENCE: "reference", T.RISING: "rising"}
TILE = L.TILE


def _code(mh, fn):
    with pytest.raises(mh.MultiHError) as ei:
        fn()
    return ei.value.code


def _planes(rng, n, nh, noise=0.7, wrong=0.1):
    """n points on nh noisy planes, models near the true ones, labels = the plane with a share of wrong ones and outliers."""
    truth = rng.integers(0, nh, size=n)
    src, dst = rng.uniform(0, 1000, size=(n, 2)), rng.uniform(0, 1000, size=(n, 2))
    H = np.ascontiguousarray(rng.normal(size=(nh, 9)))
    for k in range(nh):
        m = truth == k
        s, d, Hk, _ = R.plane_scene(rng, max(int(m.sum()), 1), noise)
        src[m], dst[m] = s[:int(m.sum())], d[:int(m.sum())]
        H[k] = Hk * (1.0 + 1e-5 * rng.normal(size=9))
    labels = truth.astype(np.int32)
    flip = rng.random(n) < wrong
    labels[flip] = rng.integers(-1, nh, size=int(flip.sum()))
    return src, dst, labels, H


def _mode(engine, term, symmetric):
    engine.set_data_term(TERMS[term])
    engine.set_residual_mode(bool(symmetric))
    engine.set_residual_scope("route" if symmetric else "score")


def _check(engine, src, dst, labels, H, cand=None, term=T.REFERENCE, symmetric=False, graph=4):
    """Both calls on this input against the twin, and the arg-min against mh_data_cost's own table; graph: k of the kNN graph,
    or (rowptr, col) hits.  cand: default every label."""
    nh = H.shape[0]
    cand = np.arange(nh, dtype=np.int32) if cand is None else np.asarray(cand, dtype=np.int32)
    engine.set_correspondences(src, dst)
    if isinstance(graph, int):
        engine.build_neighbors_knn(min(graph, src.shape[0] - 1))
    else:
        engine.set_neighbors_csr(*graph)
    engine.set_models(H)
    _mode(engine, term, symmetric)
    rp, cl, w = engine.get_sym_graph()
    alt, alt_cost, own_cost = engine.best_alternative(labels)
    want = L.best_alternative(src, dst, labels, H, LAM, THR2, term, symmetric)
    assert np.array_equal(alt, want[0]), np.flatnonzero(alt != want[0])[:10]
    assert np.array_equal(alt_cost, want[1]) and np.array_equal(own_cost, want[2])
    table = engine.data_cost().astype(np.int64).reshape(src.shape[0], nh + 1)
    by_table = L.best_alternative(src, dst, labels, H, LAM, THR2, term, symmetric, table=table)
    assert np.array_equal(alt, by_table[0]) and np.array_equal(alt_cost, by_table[1]) and np.array_equal(own_cost, by_table[2])
    delta, parts, status, alt_out = engine.drop_deltas(labels, cand)
    w_delta, w_parts, w_status, _ = L.drop_deltas(src, dst, labels, H, cand, rp, cl, w, LAM, THR2, term, symmetric)
    assert np.array_equal(alt_out, alt)
    assert np.array_equal(status, w_status), (status, w_status)
    assert np.array_equal(parts, w_parts), (parts, w_parts)
    assert np.array_equal(delta, w_delta), (delta, w_delta)
    ok = status == L.OK
    assert (delta[~ok] == L.NO_DELTA).all() and (delta[ok] == parts[ok, 2] - parts[ok, 1] + parts[ok, 4] - parts[ok, 3]).all()
    return (alt, alt_cost, own_cost), (delta, parts, status), (rp, cl, w)


# ---- 1. site and tile edges of the arg-min ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 255, 256, 257, 513])
def test_site_edges(engine, n):
    rng = np.random.default_rng(n)
    src, dst, labels, H = _planes(rng, n, 3)
    (alt, _, _), _, _ = _check(engine, src, dst, labels, H)
    assert (alt != labels).all()


@pytest.mark.parametrize("nh", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_tile_edges(engine, nh):
    rng = np.random.default_rng(1000 + nh)
    src, dst, labels, H = _planes(rng, 300, nh)
    if nh > 1:
        # six sites exactly on plane 0, three under label 0 and three under the last label of the last tile, whose model is
        # model 0: under the rising term both cost them 0, so the last label is met from label 0 and meets it
        q = np.concatenate([src[:6], np.ones((6, 1))], axis=1) @ H[0].reshape(3, 3).T
        dst[:6] = q[:, :2] / q[:, 2:3]
        labels[:6] = [0, 0, 0, nh - 1, nh - 1, nh - 1]
        H[nh - 1] = H[0]
    (alt, alt_cost, _), _, _ = _check(engine, src, dst, labels, H, term=T.RISING)
    if nh > 1:
        assert alt[:6].tolist() == [nh - 1] * 3 + [0] * 3 and (alt_cost[:6] == 0).all()


def test_unused_labels_in_the_middle_of_a_tile(engine):
    rng = np.random.default_rng(77)
    nh = TILE + 9
    src, dst, labels, H = _planes(rng, 300, nh)
    hole = (labels >= 20) & (labels < 41)
    H[20:41] = H[labels[~hole & (labels >= 0)][0]]           # tempting models that nobody uses
    labels[hole] = -1
    (alt, _, _), (_, _, status), _ = _check(engine, src, dst, labels, H)
    assert not ((alt >= 20) & (alt < 41)).any() and (status[20:41] == L.EMPTY).all()
    assert (alt[labels < 0] >= 0).any()


def test_the_tie_rule_and_sites_without_a_candidate(engine):
    rng = np.random.default_rng(78)
    src, dst, labels, H = _planes(rng, 300, 4, wrong=0.0)
    H[2] = H[3] = H[1]                                       # equal integer costs by construction
    labels[:8] = [1, 2, 3, 1, 2, 3, -1, -1]
    (alt, alt_cost, _), _, _ = _check(engine, src, dst, labels, H)
    on0 = np.flatnonzero((labels == 0) & (alt >= 0))
    assert not np.isin(alt[on0], (2, 3)).any()
    # every model beyond the threshold: the outlier wins; an outlier's alternative is the lowest used label
    far = H.copy()
    far[:, 2] += 1.0e5 * far[:, 8]
    (alt, alt_cost, own), (delta, parts, status), _ = _check(engine, src, dst, labels, far, term=T.RISING)
    assert (alt[labels >= 0] == -1).all() and (alt_cost[labels >= 0] == OUTLIER).all() and (own[labels >= 0] == 2 * OUTLIER).all()
    assert (alt[labels < 0] == 0).all() and (alt_cost[labels < 0] == 2 * OUTLIER).all()
    assert (parts[:, 2] - parts[:, 1] == -OUTLIER * parts[:, 0]).all()
    # nobody carries a label: no candidate anywhere
    nobody = np.full(300, -1, dtype=np.int32)
    (alt, alt_cost, own), (_, _, status), _ = _check(engine, src, dst, nobody, H)
    assert (alt == -1).all() and (alt_cost == OUTLIER).all() and (own == OUTLIER).all() and (status == L.EMPTY).all()


# ---- 2. member-loop edges of the drop ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 4095, 4096, 4097, 8193])
def test_member_loop_edges(engine, n):
    rng = np.random.default_rng(n)
    src, dst, labels, H = _planes(rng, n, 3)
    _, (_, parts, status), _ = _check(engine, src, dst, labels, H)
    assert (status == L.OK).all() and (parts[:, 3] > 0).all()


def test_members_in_one_lane(engine):
    rng = np.random.default_rng(21)
    n = 1280
    src, dst, labels, H = _planes(rng, n, 2, wrong=0.0)
    lane = np.array([7, 263, 519, 775, 1031])
    labels[:] = 0
    labels[lane] = 1
    _, (_, parts, status), _ = _check(engine, src, dst, labels, H)
    assert status.tolist() == [L.OK, L.OK] and parts[:, 0].tolist() == [n - 5, 5]


def test_a_row_longer_than_a_workgroup(engine):
    rng = np.random.default_rng(31)
    n = 300
    src, dst, labels, H = _planes(rng, n, 3)
    engine.set_correspondences(src, dst)
    assert engine.build_neighbors_radius(1e9) > 256 * n
    rp, cl, w = engine.get_sym_graph()
    assert np.diff(rp).min() == n - 1
    engine.set_models(H)
    delta, parts, status, alt = engine.drop_deltas(labels, [0, 1, 2])
    want = L.drop_deltas(src, dst, labels, H, [0, 1, 2], rp, cl, w, LAM, THR2, T.REFERENCE, False)
    assert np.array_equal(status, want[2]) and np.array_equal(parts, want[1]) and np.array_equal(delta, want[0]) and np.array_equal(alt, want[3])
    for k in range(3):                                       # every pair is adjacent: before the drop k's members are cut from all others
        c = int((labels == k).sum())
        assert parts[k, 3] == 50 * int(w[0]) * c * (n - c)


def test_a_directed_hit_list_with_multiplicities(engine):
    rng = np.random.default_rng(32)
    n = 400
    src, dst, labels, H = _planes(rng, n, 3)
    hits = [list(rng.choice(n, size=3, replace=False)) for _ in range(n)]
    for i in range(0, n, 5):
        if i not in hits[int(hits[i][0])]:
            hits[int(hits[i][0])].append(i)                  # a mutual hit: w = 2
    for i in range(0, n, 11):
        hits[i].append(i)                                    # a self hit
    hits[17] = []
    hits = [[q for q in h if q != 17] for h in hits]         # site 17: isolated
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(h) for h in hits])
    col = np.array([q for h in hits for q in h], dtype=np.int32)
    _, (_, parts, status), (rp, cl, w) = _check(engine, src, dst, labels, H, graph=(rowptr, col))
    assert {1, 2} <= set(np.unique(w).tolist()) and rp[18] == rp[17]
    assert (status == L.OK).all() and (parts[:, 3] > 0).all()


def test_a_label_that_neighbours_only_itself(engine):
    rng = np.random.default_rng(33)
    n = 360
    src, dst, labels, H = _planes(rng, n, 4)
    island = np.arange(40, 70)
    labels[labels == 3] = 2
    labels[island] = 3
    hits = []
    for i in range(n):
        pool = island if 40 <= i < 70 else np.setdiff1d(np.arange(n), island)
        hits.append([int(q) for q in rng.choice(pool, size=3, replace=False) if q != i])
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(h) for h in hits])
    col = np.array([q for h in hits for q in h], dtype=np.int32)
    _, (_, parts, status), _ = _check(engine, src, dst, labels, H, graph=(rowptr, col))
    assert status[3] == L.OK and parts[3, 0] == 30 and parts[3, 3] == 0


# ---- 3. both data terms x both errors, and the contract on the device -----------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("term", [T.REFERENCE, T.RISING])
def test_both_data_terms_and_both_errors_with_the_contract(engine, term, symmetric):
    rng = np.random.default_rng(7 * 513)
    src, dst, labels, H = _planes(rng, 513, 3)
    H[1] = H[0] * (1.0 + 1e-6 * rng.normal(size=9))          # two models of one plane: members with somewhere to go
    (alt, _, _), (delta, parts, status), g = _check(engine, src, dst, labels, H, term=term, symmetric=symmetric)
    assert (status == L.OK).all()
    before = engine.labeling_energy(labels)
    assert before == M.labeling_energy(src, dst, labels, H, *g, LAM, THR2, term, symmetric)
    moved = 0
    for k in range(3):
        lab2 = L.labels_after_drop(labels, k, alt)
        after = engine.labeling_energy(lab2)
        assert after[0] - before[0] == delta[k], (k, after, before, delta[k])
        assert after[1] - before[1] == parts[k, 2] - parts[k, 1] and after[2] - before[2] == parts[k, 4] - parts[k, 3]
        moved += int((lab2[labels == k] >= 0).sum())
    assert moved > 0


# ---- 4. arguments and state -----------------------------------------------------------------------------------------------------------
def test_arguments(engine, mh):
    rng = np.random.default_rng(61)
    n = 300
    src, dst, labels, H = _planes(rng, n, 3)
    lib, ip, lp = engine.lib, C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    lab = np.ascontiguousarray(labels)
    cd = np.array([0, 2], dtype=np.int32)
    alt = np.zeros(n, np.int32)
    dl, st = np.zeros(2, np.int64), np.zeros(2, np.int32)
    best = lambda h, l, a: lib.mh_best_alternative(h, l, a, None, None)
    drop = lambda h, l, c, k, d, s: lib.mh_drop_deltas(h, l, c, k, d, None, s, None)
    args = (lab.ctypes.data_as(ip), cd.ctypes.data_as(ip), 2, dl.ctypes.data_as(lp), st.ctypes.data_as(ip))
    assert drop(None, *args) == INVALID and best(None, args[0], alt.ctypes.data_as(ip)) == INVALID
    # NOT_SET: no correspondences, no models, (the deltas) no graph
    assert _code(mh, lambda: engine.drop_deltas(labels, cd)) == NOT_SET and _code(mh, lambda: engine.best_alternative(labels)) == NOT_SET
    engine.set_correspondences(src, dst)
    assert _code(mh, lambda: engine.drop_deltas(labels, cd)) == NOT_SET and _code(mh, lambda: engine.best_alternative(labels)) == NOT_SET
    engine.set_models(H)
    assert _code(mh, lambda: engine.drop_deltas(labels, cd)) == NOT_SET
    want = L.best_alternative(src, dst, labels, H, LAM, THR2, T.REFERENCE, False)
    got = engine.best_alternative(labels)                    # needs no graph
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    engine.build_neighbors_knn(4)
    assert drop(engine._h, *args) == 0 and st.tolist() == [L.OK, L.OK]
    # INVALID: null arrays, ncand out of range, a bad candidate, a label outside -1 .. Nh-1
    for hole in range(4):
        a = list(args)
        a[hole if hole < 2 else hole + 1] = None
        assert drop(engine._h, *a) == INVALID, hole
    assert best(engine._h, None, alt.ctypes.data_as(ip)) == INVALID and best(engine._h, args[0], None) == INVALID
    assert drop(engine._h, args[0], args[1], -1, args[3], args[4]) == INVALID
    assert drop(engine._h, args[0], args[1], 4, args[3], args[4]) == INVALID
    for bad in (3, -1, 1 << 20):
        assert _code(mh, lambda: engine.drop_deltas(labels, [0, bad])) == INVALID, bad
    for bad in (3, -2, 1 << 20):
        wrong = labels.copy()
        wrong[5] = bad
        assert _code(mh, lambda: engine.drop_deltas(wrong, cd)) == INVALID, bad
        assert _code(mh, lambda: engine.best_alternative(wrong)) == INVALID, bad
    # ncand == 0: MH_OK, null arrays allowed, nothing comes back; ncand == Nh and a label named twice are fine
    assert lib.mh_drop_deltas(engine._h, None, None, 0, None, None, None, None) == 0
    out = engine.drop_deltas(labels, np.zeros(0, np.int32))
    assert out[0].size == 0 and out[1].shape == (0, 5) and out[2].size == 0
    twice = engine.drop_deltas(labels, [1, 1, 0])
    assert twice[0][0] == twice[0][1] and (twice[2] == L.OK).all()
    # a candidate without a member: EMPTY, LLONG_MAX, and the caller's row of parts stays
    lab2 = np.ascontiguousarray(np.where(labels == 2, -1, labels).astype(np.int32))
    raw_parts = np.full((2, 5), -99, dtype=np.int64)
    rc = lib.mh_drop_deltas(engine._h, lab2.ctypes.data_as(ip), args[1], 2, args[3], raw_parts.ctypes.data_as(lp), args[4], None)
    assert rc == 0 and st.tolist() == [L.OK, L.EMPTY] and dl[1] == L.NO_DELTA and (raw_parts[1] == -99).all() and raw_parts[0, 0] == (lab2 == 0).sum()


def test_the_calls_change_nothing_in_the_engine(engine, mh):
    sc = mh.synth.make_scene(600, 4, seed=5, knn=8)
    H = np.ascontiguousarray(sc.H_true / np.linalg.norm(sc.H_true, axis=1, keepdims=True))
    labels = np.where(sc.gt_label >= 0, sc.gt_label, -1).astype(np.int32)
    engine.set_correspondences(sc.src, sc.dst)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    engine.set_models(H)
    engine.data_cost(fetch=False)
    want = engine.expand()
    engine.set_models(H)
    engine.data_cost(fetch=False)
    first = engine.drop_deltas(labels, np.arange(4))
    alts = engine.best_alternative(labels)
    e0 = engine.labeling_energy(labels)
    assert (first[2] == L.OK).all() and np.array_equal(first[3], alts[0])
    assert engine.model_count == 4 and np.array_equal(engine.get_models().view(np.uint64), H.view(np.uint64))
    got = engine.expand()                                    # no mh_data_cost in between: the table is still fresh
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    again = engine.drop_deltas(labels, np.arange(4))
    assert all(np.array_equal(a, b) for a, b in zip(again, first)) and engine.labeling_energy(labels) == e0


# ---- 5. Process() ----------------------------------------------------------------------------------------------------------------------
def _host(mh):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_merge_mode.argtypes = [C.c_int]
    host.mhh_set_merge_mode.restype = None
    host.mhh_set_label_cost.argtypes = [C.c_double]
    host.mhh_set_label_cost.restype = None
    host.mhh_set_neighbourhood.argtypes = [C.c_int, C.c_double]
    host.mhh_set_neighbourhood.restype = None
    return host


def _run_process(host, sc, init_H):
    dp = C.POINTER(C.c_double)
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((64, 9))
    it, en = C.c_int(-1), C.c_double(-1)
    src, dst, aff, F, e2, init = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff, sc.F, sc.e2, init_H))
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, F.ctypes.data_as(dp),
                             e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5), 20,
                             C.c_ulonglong(5), 4000, 16, 0, init.ctypes.data_as(dp), init.shape[0], labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 64, C.byref(it), C.byref(en), None, 0, 4)
    mlog, dlog = np.zeros((64, 9), dtype=np.int64), np.zeros((64, 9), dtype=np.int64)
    nm = host.mhh_get_merge_log(mlog.ctypes.data_as(C.POINTER(C.c_longlong)), 64)
    nd = host.mhh_get_drop_log(dlog.ctypes.data_as(C.POINTER(C.c_longlong)), 64)
    return k, labels, Hout[:max(k, 0)].copy(), mlog[:min(nm, 64)].copy(), dlog[:min(nd, 64)].copy()


def test_process_drops_the_spurious_label(mh, engine_lib):
    """Two planes of some 600 points each; initial models as in test_process_joins_two_halves_of_a_plane (plane B's true model, two
    models that each fit one half of plane A) and one more, the refit of a 20-point patch of plane A (label_cost_scene;
    tests/test_label_cost_cpu.py holds the twin's margins on the truth labeling plus the patch).  After the first LabelingStep
    plane A is under three labels, and the step of iteration 2 evaluates 6 pairs.  Measured, per cost:
      0 (MERGE_ENERGY alone)  one join (delta -2 983), 3 models go on; no drop log.
      40 outliers' worth (beta 196 040), the figure the mode was specified with: a second join is below beta (delta +8 481, a label
         of plane A with the one partner the first join left it, plane B) and is taken — the joins run first, so no label is
         left to drop: 2 joins, no drop, two models.
      1 outlier's worth (beta 4 901): that join is refused and the drop does what it is for — the third label of plane A cannot
         be joined in the same step (no label twice); its 540 members all take the other label of their plane, none the outlier
         label, delta -3 315: E_after 2 469 602 == E_before 2 472 917 + delta, a second mh_labeling_energy call; two models.
    So the asserted run is the one at cost 1 (exactly one accepted drop, E_after == E_before + delta, two models at the end), and
    the run at 40 is held to what it does.  With label cost 0 the drop log is empty and labels, models and merge log are those
    of MERGE_ENERGY alone, bit for bit; a negative, a non-finite cost, and a positive one without MERGE_ENERGY make Process()
    fail."""
    host = _host(mh)
    sc, init, _ = L.label_cost_scene(mh)
    try:
        host.mhh_set_neighbourhood(8, 0.0)
        host.mhh_set_merge_mode(1)
        k0, lab0, H0, mlog0, dlog0 = _run_process(host, sc, init)
        assert k0 >= 2 and dlog0.shape[0] == 0
        host.mhh_set_label_cost(0.0)
        k1, lab1, H1, mlog1, dlog1 = _run_process(host, sc, init)
        assert k1 == k0 and np.array_equal(lab1, lab0) and np.array_equal(H1.view(np.uint64), H0.view(np.uint64))
        assert np.array_equal(mlog1, mlog0) and dlog1.shape[0] == 0
        host.mhh_set_label_cost(1.0)
        k, lab, H, mlog, dlog = _run_process(host, sc, init)
        print("merge log\n", mlog, "\ndrop log\n", dlog)
        assert dlog.shape[0] >= 1 and (dlog[:, 6] == OUTLIER).all() and np.array_equal(dlog[:, 0], mlog[:, 0])
        accepted = dlog[dlog[:, 2] >= 0]
        assert accepted.shape[0] == 1
        iteration, candidates, dropped, members, to_outlier, delta, beta, e_before, e_after = accepted[0].tolist()
        assert delta - beta < 0 and e_after == e_before + delta and 1 <= members and 0 <= to_outlier <= members and 0 <= dropped < 4
        assert candidates == 3
        for rec in dlog[dlog[:, 2] < 0].tolist():
            assert rec[3] == 0 and rec[4] == 0 and rec[5] == 0 and rec[8] == rec[7]
        first = mlog[mlog[:, 0] == iteration][0].tolist()
        assert first[3] == 1 and first[4] == 0 and first[7] == e_after and first[7] == first[5] + first[6]      # E_start = E_before + sum_delta
        assert k == 2 and set(np.unique(lab[lab >= 0]).tolist()) == {0, 1} and np.isfinite(H).all()
        on_a = lab[sc.gt_label == 0]
        assert np.bincount(on_a[on_a >= 0], minlength=2).max() >= 0.95 * on_a.size
        # the specified 40: the cheap join with the wrong plane comes first, no drop is left
        host.mhh_set_label_cost(40.0)
        k40, lab40, H40, mlog40, dlog40 = _run_process(host, sc, init)
        print("at 40: merge log\n", mlog40, "\ndrop log\n", dlog40)
        assert k40 == 2 and (dlog40[:, 6] == 40 * OUTLIER).all() and (dlog40[:, 2] < 0).all() and mlog40[0, 3] == 2
        for bad in (-1.0, float("nan"), float("inf")):
            host.mhh_set_label_cost(bad)
            assert _run_process(host, sc, init)[0] == -1, bad
        host.mhh_set_label_cost(40.0)
        host.mhh_set_merge_mode(0)                           # a positive cost without MERGE_ENERGY
        assert _run_process(host, sc, init)[0] == -1
    finally:
        host.mhh_set_label_cost(0.0)
        host.mhh_set_merge_mode(-1)
        host.mhh_set_neighbourhood(0, 0.0)


def test_the_harness_flag_on_the_route_without_f(mh, engine_lib, tmp_path):
    """multih_harness --merge energy --label-cost on the point-only, epipolar-free route (three moving planes): no F is needed."""
    import subprocess
    import reestimate_dlt_numpy as D
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    sc = D.three_motions(1200)
    corr, out = tmp_path / "points.txt", tmp_path / "points.out"
    np.savetxt(corr, np.concatenate([sc.src, sc.dst], axis=1), fmt="%.17g")
    r = subprocess.run([harness, str(corr), str(out), "--points", "--no-epipolar", "--merge", "energy", "--label-cost", "10"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Energy merges:" in r.stdout and "Label cost: beta " in r.stdout and "candidates evaluated" in r.stdout
    res = np.loadtxt(out, ndmin=2)
    assert res.shape == (sc.n, 5) and len(set(int(v) for v in res[:, 4]) - {-1}) >= 2
    # a cost without the energy-tested merge: Process() fails with a message
    r = subprocess.run([harness, str(corr), str(out), "--points", "--no-epipolar", "--label-cost", "10"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "label cost" in r.stderr
