"""mh_merge_deltas and mh_labeling_energy on the GPU (csrc/merge_energy.hip: k_merge_pair, k_labeling_energy) and the MERGE_ENERGY
mode of MultiH::MergingStep.  Everything integer is compared EXACTLY with the twin (tests/merge_energy_numpy.py) and every H_out
row BIT FOR BIT with refit_h_numpy.fit over the union: at the stride and trip edges of the member loop, at the membership edges,
on long and on irregular graph rows, against the existing kernels (mh_data_cost's table, mh_expand's energy), with many labels,
at the argument and state edges, on a scene with one split plane, and through Process()."""
import ctypes as C
import os

import numpy as np
import pytest

import data_term_numpy as T
import merge_energy_numpy as M
import refit_h_numpy as R

pytestmark = pytest.mark.gpu

INVALID, NOT_SET = -2, -4
LAM, THR2 = 0.5, 2.2 ** 2                                 # the engine fixture's lambda and thr_hom^2
TERMS = {T.REFERENCE: "reference", T.RISING: "rising"}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _code(mh, fn):
    with pytest.raises(mh.MultiHError) as ei:
        fn()
    return ei.value.code


def _all_pairs(nh):
    return np.array([(a, b) for a in range(nh) for b in range(a + 1, nh)], dtype=np.int32)


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


def _check(engine, src, dst, labels, H, pairs, term=T.REFERENCE, symmetric=False, graph=4):
    """mh_merge_deltas and mh_labeling_energy on this input against the twin; graph: k of the kNN graph, or (rowptr, col) hits."""
    engine.set_correspondences(src, dst)
    if isinstance(graph, int):
        engine.build_neighbors_knn(min(graph, src.shape[0] - 1))
    else:
        engine.set_neighbors_csr(*graph)
    engine.set_models(H)
    _mode(engine, term, symmetric)
    rp, cl, w = engine.get_sym_graph()
    sentinel = np.full((len(pairs), 9), 12345.0)
    got_H, delta, parts, status = engine.merge_deltas(labels, pairs, H_out=sentinel.copy())
    want_H, want_delta, want_parts, want_status = M.merge_deltas(src, dst, labels, H, pairs, rp, cl, w, LAM, THR2, term, symmetric)
    assert np.array_equal(status, want_status), (status, want_status)
    assert np.array_equal(delta, want_delta), (delta, want_delta)
    assert np.array_equal(parts, want_parts), (parts, want_parts)
    ok = status == M.OK
    assert np.array_equal(_bits(got_H[ok]), _bits(want_H[ok])), np.flatnonzero((_bits(got_H) != _bits(want_H)).any(axis=1) & ok)
    assert np.array_equal(_bits(got_H[~ok]), _bits(sentinel[~ok]))
    assert (delta[~ok] == M.NO_DELTA).all() and (delta[ok] == parts[ok, 2] - parts[ok, 1] - parts[ok, 3]).all()
    return got_H, delta, parts, status, (rp, cl, w)


# ---- 1. stride and trip edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 255, 256, 257, 513, 4095, 4096, 4097, 8193])
def test_stride_and_trip_edges(engine, n):
    rng = np.random.default_rng(n)
    src, dst, labels, H = _planes(rng, n, 3)
    _, _, parts, status, _ = _check(engine, src, dst, labels, H, _all_pairs(3))
    if n >= 255:
        assert (status == M.OK).all() and (parts[:, 3] > 0).all()


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("term", [T.REFERENCE, T.RISING])
@pytest.mark.parametrize("n", [513, 4097])
def test_both_data_terms_and_both_errors(engine, n, term, symmetric):
    rng = np.random.default_rng(7 * n)
    src, dst, labels, H = _planes(rng, n, 3)
    _, _, parts, status, g = _check(engine, src, dst, labels, H, _all_pairs(3), term, symmetric)
    assert (status == M.OK).all()
    valid = np.where(labels < 3, labels, -1)
    assert engine.labeling_energy(valid) == M.labeling_energy(src, dst, valid, H, *g, LAM, THR2, term, symmetric)


# ---- 2. membership -----------------------------------------------------------------------------------------------------------
def test_one_side_in_one_lane(engine):
    rng = np.random.default_rng(21)
    n = 1280
    src, dst, labels, H = _planes(rng, n, 2, wrong=0.0)
    lane = np.array([7, 263, 519, 775, 1031])
    labels[:] = 0
    labels[lane] = 1
    _, _, parts, status, _ = _check(engine, src, dst, labels, H, [[0, 1]])
    assert status.tolist() == [M.OK] and parts[0, 0] == n


def test_small_sets_empty_sides_and_labels_of_nobody(engine):
    rng = np.random.default_rng(22)
    n = 700
    src, dst, _, H = _planes(rng, n, 6, wrong=0.0)
    labels = np.full(n, -1, dtype=np.int32)
    perm = rng.permutation(n)
    labels[perm[0:2]] = 0; labels[perm[2:4]] = 1            # 2 + 2: fitted
    labels[perm[4:5]] = 2; labels[perm[5:7]] = 3            # 1 + 2: no fit
    labels[perm[7:300]] = 4                                 # label 5 has no member
    labels[perm[300:320]] = 6                               # Nh
    labels[perm[320:340]] = 1 << 20
    pairs = [[0, 1], [2, 3], [4, 5], [0, 5], [3, 4], [0, 4]]
    engine.set_correspondences(src, dst)
    engine.build_neighbors_knn(4)
    engine.set_models(H)
    _, delta, parts, status, g = _check(engine, src, dst, labels, H, pairs)
    assert status.tolist() == [M.OK, M.NO_FIT, M.EMPTY, M.EMPTY, M.OK, M.OK]
    assert parts[:, 0].tolist() == [4, 0, 0, 0, 295, 295]
    # the caller's bits of `parts` stay too where a pair is not OK (through the C ABI: Engine.merge_deltas hands in zeros)
    lab, pr = np.ascontiguousarray(labels), np.ascontiguousarray(pairs, dtype=np.int32)
    raw_parts = np.full((len(pairs), 4), -99, dtype=np.int64)
    raw_delta, raw_status = np.zeros(len(pairs), np.int64), np.zeros(len(pairs), np.int32)
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    rc = engine.lib.mh_merge_deltas(engine._h, lab.ctypes.data_as(ip), pr.ctypes.data_as(ip), len(pairs), None, raw_delta.ctypes.data_as(lp),
                                    raw_parts.ctypes.data_as(lp), raw_status.ctypes.data_as(ip))
    assert rc == 0 and np.array_equal(raw_status, status) and np.array_equal(raw_delta, delta)
    assert (raw_parts[status != M.OK] == -99).all() and np.array_equal(raw_parts[status == M.OK], parts[status == M.OK])
    # labels of nobody are nobody's: as outliers they give the same answers
    same = np.where((labels >= 0) & (labels < 6), labels, -1)
    again = engine.merge_deltas(same, pairs)
    assert np.array_equal(again[1], delta) and np.array_equal(again[2], parts) and np.array_equal(again[3], status)


# ---- 3. graph edges ----------------------------------------------------------------------------------------------------------
def test_rows_longer_than_a_workgroup(engine):
    rng = np.random.default_rng(31)
    n = 300
    src, dst, labels, H = _planes(rng, n, 3)
    engine.set_correspondences(src, dst)
    assert engine.build_neighbors_radius(1e9) > 256 * n
    rp, cl, w = engine.get_sym_graph()
    assert np.diff(rp).min() == n - 1
    engine.set_models(H)
    got = engine.merge_deltas(labels, _all_pairs(3))
    want = M.merge_deltas(src, dst, labels, H, _all_pairs(3), rp, cl, w, LAM, THR2, T.REFERENCE, False)
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    for k, (a, b) in enumerate(_all_pairs(3)):
        assert got[2][k, 3] == 50 * int(w[0]) * int((labels == a).sum()) * int((labels == b).sum())       # every pair is adjacent
    valid = np.where(labels < 3, labels, -1)
    assert engine.labeling_energy(valid) == M.labeling_energy(src, dst, valid, H, rp, cl, w, LAM, THR2, T.REFERENCE, False)


def test_directed_hit_lists(engine):
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
    _, _, parts, status, (rp, cl, w) = _check(engine, src, dst, labels, H, _all_pairs(3), graph=(rowptr, col))
    assert {1, 2} <= set(np.unique(w).tolist()) and rp[18] == rp[17]
    assert (status == M.OK).all() and (parts[:, 3] > 0).all()
    valid = np.where(labels < 3, labels, -1)
    assert engine.labeling_energy(valid) == M.labeling_energy(src, dst, valid, H, rp, cl, w, LAM, THR2, T.REFERENCE, False)


# ---- 4. against the existing kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [False, True])
def test_data_old_is_the_data_cost_tables_sum(engine, symmetric):
    rng = np.random.default_rng(41)
    src, dst, labels, H = _planes(rng, 900, 4)
    pairs = _all_pairs(4)
    _, _, parts, status, _ = _check(engine, src, dst, labels, H, pairs, T.RISING, symmetric)
    cost = engine.data_cost().astype(np.int64)
    for k, (a, b) in enumerate(pairs):
        m = np.flatnonzero((labels == a) | (labels == b))
        assert parts[k, 1] == cost[m, labels[m] + 1].sum()


@pytest.mark.parametrize("term", [T.REFERENCE, T.RISING])
def test_the_energy_of_expansions_labels_and_the_contract(engine, mh, term):
    sc = mh.synth.make_scene(600, 4, seed=3, knn=8)
    engine.set_correspondences(sc.src, sc.dst)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    H = np.ascontiguousarray(sc.H_true / np.linalg.norm(sc.H_true, axis=1, keepdims=True))
    engine.set_models(H)
    _mode(engine, term, False)
    engine.data_cost(fetch=False)
    lab, energy, _ = engine.expand()
    labels = (lab - 1).astype(np.int32)
    before = engine.labeling_energy(labels)
    assert before[0] == energy and before[0] == before[1] + before[2]
    # the contract: relabel b -> a, model a = H_ab, and the energy moves by delta
    pairs = _all_pairs(4)
    Hs, delta, parts, status = engine.merge_deltas(labels, pairs)
    assert (status == M.OK).any()
    for k in np.flatnonzero(status == M.OK):
        lab2, H2 = M.apply_merges(labels, H, pairs, Hs, [int(k)])
        engine.set_models(H2)
        after = engine.labeling_energy(lab2)
        assert after[0] - before[0] == delta[k] and after[2] - before[2] == -parts[k, 3], (pairs[k], after, before, delta[k])
    engine.set_models(H)
    assert engine.labeling_energy(labels) == before


# ---- 5. many labels ----------------------------------------------------------------------------------------------------------
def test_three_hundred_labels_six_hundred_pairs(engine):
    rng = np.random.default_rng(51)
    n, nh = 2048, 300
    src, dst, labels, _ = _planes(rng, n, 6, wrong=0.0)
    labels = (labels + 6 * rng.integers(0, nh // 6, size=n)).astype(np.int32)
    H = np.ascontiguousarray(rng.normal(size=(nh, 9)))
    allp = _all_pairs(nh)
    pairs = allp[np.sort(rng.permutation(len(allp))[:600])]
    _, _, _, status, _ = _check(engine, src, dst, labels, H, pairs)
    assert (status == M.OK).sum() > 500


# ---- 6. arguments and state ----------------------------------------------------------------------------------------------------
def test_arguments(engine, mh):
    rng = np.random.default_rng(61)
    n = 300
    src, dst, labels, H = _planes(rng, n, 3)
    lib, ip, lp = engine.lib, C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    lab = np.ascontiguousarray(labels)
    pr = np.array([[0, 1]], dtype=np.int32)
    dl, st, en = np.zeros(1, np.int64), np.zeros(1, np.int32), C.c_longlong(0)
    raw = lambda h, l, p, k, d, s: lib.mh_merge_deltas(h, l, p, k, None, d, None, s)
    args = (lab.ctypes.data_as(ip), pr.ctypes.data_as(ip), 1, dl.ctypes.data_as(lp), st.ctypes.data_as(ip))
    assert raw(None, *args) == INVALID and lib.mh_labeling_energy(None, lab.ctypes.data_as(ip), C.byref(en), None) == INVALID
    # NOT_SET: no correspondences, no models, no graph
    assert _code(mh, lambda: engine.merge_deltas(labels, pr)) == NOT_SET and _code(mh, lambda: engine.labeling_energy(labels)) == NOT_SET
    engine.set_correspondences(src, dst)
    assert _code(mh, lambda: engine.merge_deltas(labels, pr)) == NOT_SET and _code(mh, lambda: engine.labeling_energy(labels)) == NOT_SET
    engine.set_models(H)
    assert _code(mh, lambda: engine.merge_deltas(labels, pr)) == NOT_SET and _code(mh, lambda: engine.labeling_energy(labels)) == NOT_SET
    engine.build_neighbors_knn(4)
    assert raw(engine._h, *args) == 0 and st[0] == M.OK
    # INVALID: null arrays with npairs > 0, npairs out of range, bad pairs, a label outside -1 .. Nh-1 for the energy
    for hole in range(4):
        a = list(args)
        a[hole if hole < 2 else hole + 1] = None
        assert raw(engine._h, *a) == INVALID, hole
    assert raw(engine._h, args[0], args[1], -1, args[3], args[4]) == INVALID
    assert raw(engine._h, args[0], args[1], (1 << 20) + 1, args[3], args[4]) == INVALID
    for bad in ([1, 1], [1, 0], [-1, 1], [0, 3], [2, 3]):
        assert _code(mh, lambda: engine.merge_deltas(labels, [bad])) == INVALID, bad
    for bad in (3, -2, 1 << 20):
        wrong = labels.copy()
        wrong[5] = bad
        assert _code(mh, lambda: engine.labeling_energy(wrong)) == INVALID, bad
    assert lib.mh_labeling_energy(engine._h, None, C.byref(en), None) == INVALID
    assert lib.mh_labeling_energy(engine._h, lab.ctypes.data_as(ip), None, None) == INVALID
    # npairs == 0: MH_OK, null arrays allowed, nothing comes back
    assert lib.mh_merge_deltas(engine._h, None, None, 0, None, None, None, None) == 0
    out = engine.merge_deltas(labels, np.zeros((0, 2), np.int32))
    assert out[0].shape == (0, 9) and out[1].size == 0 and out[3].size == 0


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
    got_H, delta, parts, status = engine.merge_deltas(labels, _all_pairs(4))
    e0 = engine.labeling_energy(labels)
    assert (status == M.OK).all()
    assert engine.model_count == 4 and np.array_equal(_bits(engine.get_models()), _bits(H))
    got = engine.expand()                                    # no mh_data_cost in between: the table is still fresh
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    again = engine.merge_deltas(labels, _all_pairs(4))
    assert np.array_equal(again[1], delta) and np.array_equal(_bits(again[0]), _bits(got_H)) and engine.labeling_energy(labels) == e0


# ---- 7. a scene with one plane split in two ------------------------------------------------------------------------------------
def _split_scene(mh):
    sc = mh.synth.make_scene(1500, 3, seed=7)
    labels = sc.gt_label.astype(np.int32).copy()
    on0 = np.flatnonzero(sc.gt_label == 0)
    labels[on0[sc.src[on0, 0] > np.median(sc.src[on0, 0])]] = 3
    H = np.stack([R.fit(sc.src, sc.dst, np.flatnonzero(labels == k)) for k in range(4)])
    return sc, labels, np.ascontiguousarray(H)


def test_the_split_plane_is_the_one_merge(engine, mh):
    sc, labels, H = _split_scene(mh)
    engine.set_correspondences(sc.src, sc.dst)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    engine.set_estimator("dlt")
    engine.set_models(H)
    pairs = _all_pairs(4)
    Hs, delta, parts, status = engine.merge_deltas(labels, pairs)
    assert (status == M.OK).all()
    split = [tuple(p) for p in pairs.tolist()].index((0, 3))
    assert delta[split] < 0 and (np.delete(delta, split) > 0).all(), delta
    assert M.select_merges(pairs, delta, status, 4) == [split]
    before = engine.labeling_energy(labels)[0]
    lab2, H2 = M.apply_merges(labels, H, pairs, Hs, [split])
    engine.set_models(H2)
    start = engine.labeling_energy(lab2)[0]
    assert start == before + delta[split]
    lab3, energy, _ = engine.labeling_step(True, lab2)
    assert energy <= start and lab3.min() >= -1 and lab3.max() <= 2


# ---- 8. Process() --------------------------------------------------------------------------------------------------------------
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
    log = np.zeros((64, 9), dtype=np.int64)
    records = host.mhh_get_merge_log(log.ctypes.data_as(C.POINTER(C.c_longlong)), 64)
    return k, labels, Hout[:max(k, 0)].copy(), log[:min(records, 64)].copy()


def test_process_in_both_merge_modes(mh, engine_lib):
    """The setup the mode was specified with: the three true models plus refits of plane 0's two halves.  Measured: NO join is
    accepted here, under either data term and either estimator — the first LabelingStep gives all of plane 0 to one of its
    three models, the two others keep no member and every pair with them is EMPTY (10 pairs evaluated per step, 0 accepted; the
    post-filter removes the empty models).  So on this setup E_start == E_before + sum_delta holds with sum_delta == 0;
    test_process_joins_two_halves_of_a_plane below is the run in which a join is accepted and the models change."""
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_merge_mode.argtypes = [C.c_int]
    host.mhh_set_merge_mode.restype = None
    host.mhh_set_neighbourhood.argtypes = [C.c_int, C.c_double]
    host.mhh_set_neighbourhood.restype = None
    sc = mh.synth.make_scene(1500, 3, seed=7)
    on0 = np.flatnonzero(sc.gt_label == 0)
    right = sc.src[on0, 0] > np.median(sc.src[on0, 0])
    init = np.concatenate([sc.H_true / np.linalg.norm(sc.H_true, axis=1, keepdims=True),
                           np.stack([R.fit(sc.src, sc.dst, on0[~right]), R.fit(sc.src, sc.dst, on0[right])])])
    try:
        host.mhh_set_neighbourhood(8, 0.0)
        k0, lab0, H0, log0 = _run_process(host, sc, init)
        assert k0 >= 1 and log0.shape[0] == 0
        host.mhh_set_merge_mode(0)                           # MERGE_MEAN_SHIFT set explicitly: the default, bit for bit
        k1, lab1, H1, log1 = _run_process(host, sc, init)
        assert k1 == k0 and np.array_equal(lab1, lab0) and np.array_equal(_bits(H1), _bits(H0)) and log1.shape[0] == 0
        host.mhh_set_merge_mode(1)                           # MERGE_ENERGY
        k2, lab2, H2, log = _run_process(host, sc, init)
        assert k2 >= 1 and lab2.min() >= -1 and lab2.max() == k2 - 1 and np.isfinite(H2).all()
        assert set(np.unique(lab2[lab2 >= 0]).tolist()) == set(range(k2)) or k2 == 1
        assert log.shape[0] >= 1
        for iteration, models, pairs, accepted, filtered, e_before, sum_delta, e_start, e_expansion in log.tolist():
            assert iteration >= 2 and models >= 1 and pairs == models * (models - 1) // 2 and 0 <= accepted <= models // 2
            if filtered == 0:
                assert e_start == e_before + sum_delta
            assert sum_delta <= 0
            if e_expansion >= 0:                             # (-1: the loop ended behind this MergingStep)
                assert e_expansion <= e_start
        assert (log[:-1, 8] >= 0).all()
        host.mhh_set_merge_mode(2)                           # an unknown value: Process() fails with a message
        assert _run_process(host, sc, init)[0] == -1
    finally:
        host.mhh_set_merge_mode(-1)
        host.mhh_set_neighbourhood(0, 0.0)
    k3, lab3, _, log3 = _run_process(host, sc, init)
    assert k3 == k0 and np.array_equal(lab3, lab0) and log3.shape[0] == 0


def test_process_joins_two_halves_of_a_plane(mh, engine_lib):
    """A Process() run in which MERGE_ENERGY accepts a join: the true models of planes 1 and 2 and, for plane 0, two models that
    each fit one half of it — the true homography followed by a rotation of 0.015 rad about the centroid of that half's targets,
    so the error grows to the truncation threshold (4.95 px) some 330 px away and the first LabelingStep splits the plane between
    them.  Its re-estimation makes both models good fits of their halves, and the MergingStep of iteration 2 finds the pair's
    delta negative (about minus the cut): one join, 4 -> 3 models, and E_start — a second mh_labeling_energy call on the merged
    labels and models — equals E_before + sum_delta."""
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_merge_mode.argtypes = [C.c_int]
    host.mhh_set_merge_mode.restype = None
    host.mhh_set_neighbourhood.argtypes = [C.c_int, C.c_double]
    host.mhh_set_neighbourhood.restype = None
    sc = mh.synth.make_scene(1500, 3, seed=7)
    on0 = np.flatnonzero(sc.gt_label == 0)
    right = sc.src[on0, 0] > np.median(sc.src[on0, 0])

    def half_model(side, theta):
        c = sc.dst[side].mean(axis=0)
        ct, st = np.cos(theta), np.sin(theta)
        A = np.array([[ct, -st, c[0] - ct * c[0] + st * c[1]], [st, ct, c[1] - st * c[0] - ct * c[1]], [0.0, 0.0, 1.0]])
        Hm = A @ sc.H_true[0].reshape(3, 3)
        return (Hm / np.linalg.norm(Hm)).reshape(9)

    init = np.concatenate([sc.H_true[1:] / np.linalg.norm(sc.H_true[1:], axis=1, keepdims=True),
                           np.stack([half_model(on0[~right], 0.015), half_model(on0[right], -0.015)])])
    try:
        host.mhh_set_neighbourhood(8, 0.0)
        host.mhh_set_merge_mode(1)
        k, lab, H, log = _run_process(host, sc, init)
    finally:
        host.mhh_set_merge_mode(-1)
        host.mhh_set_neighbourhood(0, 0.0)
    assert k == 3 and lab.min() >= -1 and set(np.unique(lab[lab >= 0]).tolist()) == {0, 1, 2} and np.isfinite(H).all()
    assert log.shape[0] >= 1
    iteration, models, pairs, accepted, filtered, e_before, sum_delta, e_start, e_expansion = log[0].tolist()
    assert (iteration, models, pairs, accepted, filtered) == (2, 4, 6, 1, 0)
    assert sum_delta < 0 and e_start == e_before + sum_delta and 0 <= e_expansion <= e_start
    for rec in log[1:].tolist():                             # afterwards: three models, nothing left to join
        assert rec[1] == 3 and rec[2] == 3 and rec[3] == 0 and rec[7] == rec[5]
    # plane 0 ends under one label
    own = np.bincount(lab[on0][lab[on0] >= 0], minlength=3)
    assert own.max() >= 0.95 * on0.size


def test_the_harness_flag_on_the_route_without_f(mh, engine_lib, tmp_path):
    """multih_harness --merge energy on the point-only, epipolar-free route (three moving planes): the step needs no F."""
    import subprocess
    import reestimate_dlt_numpy as D
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    sc = D.three_motions(1200)
    corr, out = tmp_path / "points.txt", tmp_path / "points.out"
    np.savetxt(corr, np.concatenate([sc.src, sc.dst], axis=1), fmt="%.17g")
    r = subprocess.run([harness, str(corr), str(out), "--points", "--no-epipolar", "--merge", "energy"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Energy merges:" in r.stdout and "pairs evaluated" in r.stdout
    res = np.loadtxt(out, ndmin=2)
    assert res.shape == (sc.n, 5) and len(set(int(v) for v in res[:, 4]) - {-1}) >= 2
