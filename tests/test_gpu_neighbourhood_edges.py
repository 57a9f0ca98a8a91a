"""The neighbourhood builders at their edges (csrc/knn.hip, csrc/graph.hip, build_knn_graph / device_sym_graph in
csrc/capi.hip), every row of every graph against a brute force that shares nothing with the kernels.

The reference is `_hit_table`: for query i the candidates j != i ranked by (d(i, j), j), the first k of them, those
beyond the radius cut; the directed table then goes through oracle.build_sym_graph (the setNeighbors multiplicity
rule).  On EXACT scenes — coordinates that are small integers or multiples of 0.25 — d is computed in int64, and the
test asserts that every squared distance (and with it every partial sum of the kernels' float32 expression) is a
float32 number, so nothing about the kernels' arithmetic is assumed: ties, duplicates and `d == r^2` are decided by
integers.  On real-valued scenes d is float32 in the documented order ((dx*dx + dy*dy) + dz*dz) + dw*dw.

Every k-NN case runs through the grid (mh_set_tuning key 31 = 1) and through the exhaustive pass (key 31 = 0), and each
of the two is compared with the reference.  All assertions are exact integer equality of rowptr, col and w."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAM = 0.5
KMAX = 32


# ---- the reference --------------------------------------------------------------------------------------------------
_RANKED = {}
_LAST_EXACT = {}                                                       # the n x n matrix of the scene asked for last


def _scene_key(src, dst):
    return hashlib.sha1(np.ascontiguousarray(src).tobytes() + np.ascontiguousarray(dst).tobytes()).hexdigest()


def _exact_distances(src, dst):
    """n x n squared distances of an exact scene as int64 counts of unit^2, and unit^2 (1 or 1/16).  Asserts that the
    scene is exact: coordinates are integers or multiples of 0.25 below 2^11, and every squared distance, counted in
    unit^2, is below 2^24 — so each square and each partial sum of the float32 expression (all of them integers of the
    same unit, none larger than the total) is a float32 number, and so is d."""
    key = _scene_key(src, dst)
    if key in _LAST_EXACT:
        return _LAST_EXACT[key]
    pv = np.concatenate([src, dst], axis=1).astype(np.float64)
    unit = 1.0 if np.array_equal(pv, np.round(pv)) else 0.25
    c = np.round(pv / unit).astype(np.int64)
    assert np.array_equal(c * unit, pv) and np.abs(pv).max() < 2 ** 11, "not an exact scene"
    D = np.zeros((pv.shape[0], pv.shape[0]), dtype=np.int64)
    for a in range(4):
        t = c[:, None, a] - c[None, :, a]
        D += t * t
    assert D.max() < 2 ** 24
    d = D.astype(np.float64) * (unit * unit)
    assert np.array_equal(d.astype(np.float32).astype(np.float64), d), "float32(d) == d must hold on an exact scene"
    D.setflags(write=False)
    _LAST_EXACT.clear()
    _LAST_EXACT[key] = (D, unit * unit)
    return D, unit * unit


def _ranked(src, dst, exact):
    """For every query the first min(33, n - 1) candidates j != i in (d, j) order, and their d (float64 for exact
    scenes, float32 otherwise).  Computed once per scene and shared."""
    key = (_scene_key(src, dst), exact)
    if key in _RANKED:
        return _RANKED[key]
    n = src.shape[0]
    m = min(KMAX + 1, n - 1)
    idx = np.empty((n, m), dtype=np.int64)
    if exact:
        D, u2 = _exact_distances(src, dst)
        assert n <= 1 << 13
        keys = (D << 13) | np.arange(n, dtype=np.int64)[None, :]       # (d, j) as one integer: d < 2^24, j < 2^13
        np.fill_diagonal(keys, np.iinfo(np.int64).max)                 # j != i
        keys = np.sort(keys, axis=1)[:, :m].copy()
        idx[:] = keys & ((1 << 13) - 1)
        dist = (keys >> 13).astype(np.float64) * u2
    else:
        pv = np.concatenate([src, dst], axis=1).astype(np.float32)
        dist = np.empty((n, m), dtype=np.float32)
        for b in range(0, n, 512):                                     # blocks of rows; every row is ranked
            diff = pv[b:b + 512, None, :] - pv[None, :, :]
            sq = diff * diff
            d = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
            rows = np.arange(d.shape[0])
            d[rows, b + rows] = np.inf
            assert np.isfinite(d).sum() == d.size - d.shape[0]
            o = np.argsort(d, axis=1, kind="stable")[:, :m]            # stable: equal d in index order
            idx[b:b + 512] = o
            dist[b:b + 512] = np.take_along_axis(d, o, axis=1)
    idx.setflags(write=False)
    dist.setflags(write=False)
    _RANKED[key] = (idx, dist)
    return _RANKED[key]


def _hit_table(src, dst, k, radius=None, exact=False):
    """The directed hit table, n x k: row i holds the first k candidates j != i in (d(i, j), j) order, -1 where the hit
    lies beyond the radius (d > float32(r) * float32(r))."""
    idx, dist = _ranked(src, dst, exact)
    assert 1 <= k <= idx.shape[1]
    table = idx[:, :k].astype(np.int32)
    if radius is not None:
        r2 = np.float32(radius) * np.float32(radius)
        table = np.where(dist[:, :k] <= r2, table, -1).astype(np.int32)
    return table


def _csr_of_table(table):
    keep = table >= 0
    rowptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    return rowptr, table[keep].astype(np.int32)


def _graph_of_table(oracle, table):
    rowptr, col = _csr_of_table(table)
    return oracle.build_sym_graph(table.shape[0], rowptr, col)


def _assert_graph(got, ref, what):
    rp, col, w = got
    rp_r, col_r, w_r = ref
    if not np.array_equal(rp, rp_r):
        i = int(np.flatnonzero(rp[1:] - rp[:-1] != rp_r[1:] - rp_r[:-1])[0])
        raise AssertionError(f"{what}: row {i} has {col[rp[i]:rp[i + 1]].tolist()} x {w[rp[i]:rp[i + 1]].tolist()}, "
                             f"reference {col_r[rp_r[i]:rp_r[i + 1]].tolist()} x {w_r[rp_r[i]:rp_r[i + 1]].tolist()}")
    bad = np.flatnonzero((col != col_r) | (w != w_r))
    if bad.size:
        i = int(np.searchsorted(rp_r, bad[0], side="right") - 1)
        raise AssertionError(f"{what}: row {i} has {col[rp[i]:rp[i + 1]].tolist()} x {w[rp[i]:rp[i + 1]].tolist()}, "
                             f"reference {col_r[rp_r[i]:rp_r[i + 1]].tolist()} x {w_r[rp_r[i]:rp_r[i + 1]].tolist()}")


def _knn_both_paths(engine, k, radius=None):
    """The graph of build_neighbors_knn through the grid (key 31 = 1) and through the exhaustive pass (key 31 = 0)."""
    got = {}
    try:
        for grid in (1, 0):
            engine.set_tuning(31, grid)
            if radius is None:
                engine.build_neighbors_knn(k)
            else:
                engine.build_neighbors_knn(k, radius=radius)
            got[grid] = engine.get_sym_graph()
    finally:
        engine.set_tuning(31, 1)
    return got


def _check_knn(engine, oracle, src, dst, k, radius=None, exact=False):
    table = _hit_table(src, dst, k, radius, exact)
    ref = _graph_of_table(oracle, table)
    got = _knn_both_paths(engine, k, radius)
    for grid in (1, 0):
        _assert_graph(got[grid], ref, f"k={k} radius={radius} key31={grid}")
    return table, ref


# ---- scenes ---------------------------------------------------------------------------------------------------------
def _exact_scene(n, seed, quarter=False):
    """Distinct-ish correspondences with exact coordinates: integers in [0, 1000) + offsets, or multiples of 0.25 in
    [0, 250) + offsets (4 x 2^20 quarter units squared stays below 2^24)."""
    rng = np.random.default_rng(seed)
    if quarter:
        src = rng.integers(0, 1000, size=(n, 2)) * 0.25
        dst = src + rng.integers(-40, 41, size=(n, 2)) * 0.25
    else:
        src = rng.integers(0, 1000, size=(n, 2)).astype(np.float64)
        dst = src + rng.integers(-30, 31, size=(n, 2))
    return src, dst


def _lattice_scene(n, per_node, seed):
    """src on a 25-pixel lattice with about `per_node` points per node, dst = src + an offset in {0, 1, 2}^2: squared
    distances inside a node are tiny integers, between nodes multiples of 625 plus a little — ties everywhere."""
    rng = np.random.default_rng(seed)
    side = max(2, int(np.ceil(np.sqrt(n / per_node))))
    src = rng.integers(0, side, size=(n, 2)) * 25.0
    dst = src + rng.integers(0, 3, size=(n, 2))
    return src, dst


REAL_N = 3073
# The exhaustive pass at n = 3073: min(16, (3073 + 1023) / 1024) = 4 slices, each ((3073 + 3) / 4 = 769 rounded up to a
# multiple of 256 =) 1024 candidates long: [0, 1024), [1024, 2048), [2048, 3072) and [3072, 3073) — ONE candidate, whose
# list is one entry and K - 1 (+inf, 0x7fffffff) pads, and for query 3072 (the candidate itself) nothing but pads.
REAL_RADIUS = {17: 60.0, 32: 85.0}
_REAL = {}


def _real_scene(synth):
    if "sc" not in _REAL:
        _REAL["sc"] = synth.make_scene(REAL_N, 4, seed=21, with_neighbours=False)
    return _REAL["sc"]


# ---- 1. all three instantiations, all rows -------------------------------------------------------------------------
@pytest.mark.parametrize("k,cut", [(1, False), (7, False), (8, False), (9, False), (16, False), (17, False), (31, False),
                                   (32, False), (17, True), (32, True)])
def test_knn_every_instantiation_every_row(engine, synth, oracle, k, cut):
    """K = 8, 16 and 32 of k_knn / k_knn_merge / k_knn_grid with k on, just below and just above each, on a real-valued
    scene whose last slice of the exhaustive pass holds one candidate (see REAL_N)."""
    sc = _real_scene(synth)
    engine.set_correspondences(sc.src, sc.dst)
    radius = REAL_RADIUS[k] if cut else None
    table, ref = _check_knn(engine, oracle, sc.src, sc.dst, k, radius)
    if cut:
        kept = int((table >= 0).sum())
        assert 0 < kept < sc.n * k, "the radius must cut some of the k nearest hits, not all"
        assert (table[:, 0] >= 0).any() and (table[:, k - 1] < 0).any()
    else:
        assert int(ref[2].sum()) == 2 * sc.n * k


# ---- 2. exact ties --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 20, 32])
def test_knn_ties_at_rank_k_are_decided_by_the_index(engine, oracle, k):
    src, dst = _lattice_scene(2049, 20, seed=5)
    _, dist = _ranked(src, dst, True)
    tied = dist[:, k - 1] == dist[:, k]
    assert tied.mean() >= 0.5, "most queries must have a tie at rank k for this case to test the tie rule"
    engine.set_correspondences(src, dst)
    _check_knn(engine, oracle, src, dst, k, exact=True)


# ---- 3. duplicates beyond k -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 32])
def test_knn_with_more_duplicates_than_k(engine, oracle, k):
    n = 1025
    src, dst = _exact_scene(n, seed=7)
    rng = np.random.default_rng(70)
    pick = rng.choice(n, size=42, replace=False)
    same, pair = pick[:40], pick[40:]
    src[same], dst[same] = (333.0, 444.0), (340.0, 450.0)              # 40 identical correspondences
    src[pair], dst[pair] = (901.0, 77.0), (905.0, 70.0)                # two identical points, nobody else at distance 0
    D, _ = _exact_distances(src, dst)
    assert ((D[same] == 0).sum(axis=1) == 40).all() and ((D[pair] == 0).sum(axis=1) == 2).all()      # self included
    idx, _ = _ranked(src, dst, True)
    assert idx[pair[0], 0] == pair[1] and idx[pair[1], 0] == pair[0]
    engine.set_correspondences(src, dst)
    table, _ = _check_knn(engine, oracle, src, dst, k, exact=True)
    others = np.sort(same)
    for i in same[:3]:                                                 # the index decides among the distance-0 ties
        assert np.array_equal(table[i, :k], others[others != i][:k])


# ---- 4. small n ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(2, 1), (3, 2), (33, 32), (65, 32), (257, 8)])
def test_knn_on_few_points(mh, engine, oracle, n, k):
    src, dst = _exact_scene(n, seed=100 + n, quarter=(n in (3, 65)))
    engine.set_correspondences(src, dst)
    _, ref = _check_knn(engine, oracle, src, dst, k, exact=True)
    if k == n - 1:                                                     # every other point: the complete graph
        rp, col, w = ref
        assert np.array_equal(rp, np.arange(n + 1) * (n - 1)) and (w == 2).all()
        assert np.array_equal(col.reshape(n, n - 1), np.array([[j for j in range(n) if j != i] for i in range(n)]))
    for grid in (1, 0):
        try:
            engine.set_tuning(31, grid)
            with pytest.raises(mh.MultiHError) as ei:
                engine.build_neighbors_knn(n)
        finally:
            engine.set_tuning(31, 1)
        assert ei.value.code == -2


# ---- 5. fewer than k candidates at finite float32 distance ---------------------------------------------------------
def test_knn_without_k_finite_candidates_fails_and_keeps_the_graph(mh, engine, oracle):
    """295 of 300 points lie 2^70 apart from everything: float32 squared distances from and to them are +inf, no
    query has 8 candidates at finite distance (the five ordinary points have four).  The build fails with
    MH_ERR_INVALID through either path and the graph set before stays.  (This case found k_knn_grid admitting
    candidates at +inf distance — they tied with its (+inf, 0x7fffffff) pads and won on the index — so that the grid
    path returned a graph where the exhaustive pass failed.)"""
    n, k = 300, 8
    rng = np.random.default_rng(9)
    src = np.zeros((n, 2)); dst = np.zeros((n, 2))
    far = np.arange(5, n)
    src[:5] = rng.integers(0, 100, size=(5, 2)); dst[:5] = src[:5] + rng.integers(-5, 6, size=(5, 2))
    src[far, 0] = (far - 4) * 2.0 ** 70; src[far, 1] = rng.integers(0, 100, size=far.size)
    dst[far, 0] = (far - 4) * 2.0 ** 70; dst[far, 1] = rng.integers(0, 100, size=far.size)
    pv = np.concatenate([src, dst], axis=1).astype(np.float32)
    assert np.isfinite(pv).all()
    with np.errstate(over="ignore"):
        diff = pv[:, None, :] - pv[None, :, :]
        sq = diff * diff
        d = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
    assert np.isinf(d[far]).sum() == far.size * (n - 1) and np.isfinite(d[:5, :5]).all() and not np.isnan(d).any()
    engine.set_correspondences(src, dst)
    deg = rng.integers(0, 6, size=n)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = rng.integers(0, n, size=int(deg.sum())).astype(np.int32)
    engine.set_neighbors_csr(rowptr, col)
    before = engine.get_sym_graph()
    _assert_graph(before, oracle.build_sym_graph(n, rowptr, col), "the graph set first")
    for grid in (1, 0):
        try:
            engine.set_tuning(31, grid)
            with pytest.raises(mh.MultiHError) as ei:
                engine.build_neighbors_knn(k)
        finally:
            engine.set_tuning(31, 1)
        assert ei.value.code == -2, grid
        _assert_graph(engine.get_sym_graph(), before, f"the earlier graph after the failed build, key31={grid}")


# ---- 6. the radius rule on d == r^2 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 257, 1025])
def test_radius_boundary_is_inclusive(engine, oracle, n):
    """r = 50 on the 25-pixel lattice: diagonal lattice neighbours with equal offsets are at d = 4 x 625 = 2500 = r^2
    exactly and are hits (the rule is <=); the same pair with dst one pixel further is at 2551 and is not."""
    r, k = 50.0, 32
    r2 = int(np.float32(r) * np.float32(r))
    assert r2 == 2500
    src, dst = _lattice_scene(n, 3, seed=60 + n)
    D, u2 = _exact_distances(src, dst)
    assert u2 == 1.0
    assert (D == r2).sum() > 0 and ((D > r2) & (D <= r2 + 51)).sum() > 0
    hit = D <= r2                                                      # the query itself included
    rowptr = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.int32)
    col = np.nonzero(hit)[1].astype(np.int32)
    engine.set_correspondences(src, dst)
    assert engine.build_neighbors_radius(r) == col.size
    got = engine.get_sym_graph()
    _assert_graph(got, oracle.build_sym_graph(n, rowptr, col), f"radius builder n={n}")
    assert (got[2] == 2).all()
    # the same r through k_hits_filter: among the k nearest there are hits at d == r^2 (kept) and beyond (cut)
    _, dist = _ranked(src, dst, True)
    assert (dist[:, :k] == r2).any() and (dist[:, :k] > r2).any()
    _check_knn(engine, oracle, src, dst, k, radius=r, exact=True)


# ---- 7. k_sym_fold: row lengths and runs ----------------------------------------------------------------------------
FOLD_N = 2100
_FOLD = {}


def _fold_scene(synth):
    if "sc" not in _FOLD:
        _FOLD["sc"] = synth.make_scene(FOLD_N, 3, seed=31, with_neighbours=False)
    return _FOLD["sc"]


def _fold_hits(row0, seed, quiet=()):
    """Site 0 hits `row0` (in the order given); nobody hits site 0 or the sites in `quiet`, which make no hits either;
    every other site makes 0 to 8 random hits."""
    rng = np.random.default_rng(seed)
    n = FOLD_N
    allowed = np.setdiff1d(np.arange(1, n), np.asarray(quiet, dtype=np.int64))
    rows = [np.asarray(row0, dtype=np.int32)]
    for i in range(1, n):
        d = 0 if i in quiet else int(rng.integers(0, 9))
        rows.append(allowed[rng.integers(0, allowed.size, size=d)].astype(np.int32))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.concatenate(rows).astype(np.int32)
    # raw row lengths as k_sym_count sees them: hits made + hits received, self hits skipped
    made = np.repeat(np.arange(n), np.diff(rowptr))
    real = made != col
    raw = np.bincount(made[real], minlength=n) + np.bincount(col[real], minlength=n)
    return rowptr, col, raw


def _load_fold(engine, sc):
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_epipolar(sc.F, sc.e2)


def _expansion_equals_oracle(engine, oracle, sc, rowptr, col, what):
    """The reverse-arc index and the row weight sums are private: the expansion on the graph is their check."""
    rng = np.random.default_rng(3)
    j = rng.integers(0, sc.H_true.shape[0])
    engine.set_models(np.concatenate([sc.H_true, sc.H_true[j:j + 1] * (1.0 + rng.normal(0, 2e-4, size=(1, 9)))], axis=0))
    cost = engine.data_cost()
    labels, energy, cycles = engine.expand()
    lab_ref, e_ref, cyc_ref, _ = oracle.expand(cost, rowptr, col, oracle.potts(LAM))
    assert energy == e_ref and cycles == cyc_ref and np.array_equal(labels, lab_ref), what


@pytest.mark.parametrize("L", [63, 64, 65, 1023, 1024, 1025])
def test_sym_fold_row_lengths(engine, synth, oracle, L):
    """A raw row of exactly L entries around the 64-lane chunk and around SYM_MAX_ROW = 1024 (1025: the host path)."""
    sc = _fold_scene(synth)
    _load_fold(engine, sc)
    rowptr, col, raw = _fold_hits(np.random.default_rng(L).permutation(np.arange(1, L + 1)), seed=L)
    assert raw[0] == L and raw.max() == L
    engine.set_neighbors_csr(rowptr, col)
    got = engine.get_sym_graph()
    _assert_graph(got, oracle.build_sym_graph(FOLD_N, rowptr, col), f"L={L}")
    assert got[0][1] == L and (got[2][:L] == 1).all()
    if L == 1024:
        _expansion_equals_oracle(engine, oracle, sc, rowptr, col, "L=1024")


def _fold_runs(case):
    if case == "one_run_of_1024":                                      # one neighbour with w == 1024; row 5 is 1024 x site 0
        return np.full(1024, 5), (5,)
    if case == "16_runs_of_64":                                        # every run ends exactly on a chunk border
        return np.repeat(np.arange(100, 1700, 100), 64), ()
    if case == "run_over_positions_60_to_70":                          # sorted row: 60 singles, 11 x site 100, 30 singles
        return np.concatenate([np.arange(1, 61), np.full(11, 100), np.arange(101, 131)]), ()
    raise ValueError(case)


@pytest.mark.parametrize("case", ["one_run_of_1024", "16_runs_of_64", "run_over_positions_60_to_70"])
def test_sym_fold_runs_across_chunk_borders(engine, synth, oracle, case):
    sc = _fold_scene(synth)
    _load_fold(engine, sc)
    row0, quiet = _fold_runs(case)
    s = np.sort(row0)
    if case == "run_over_positions_60_to_70":
        assert (s[60:71] == 100).all() and s[59] != 100 and s[71] != 100
    rowptr, col, raw = _fold_hits(np.random.default_rng(17).permutation(row0), seed=len(case), quiet=quiet)
    assert raw[0] == row0.size and raw.max() <= 1024, "the build must stay on the device path"
    engine.set_neighbors_csr(rowptr, col)
    got = engine.get_sym_graph()
    _assert_graph(got, oracle.build_sym_graph(FOLD_N, rowptr, col), case)
    rp, cl, w = got
    if case == "one_run_of_1024":
        assert raw[5] == 1024
        assert cl[rp[0]:rp[1]].tolist() == [5] and w[rp[0]:rp[1]].tolist() == [1024]
        assert cl[rp[5]:rp[6]].tolist() == [0] and w[rp[5]:rp[6]].tolist() == [1024]
        _expansion_equals_oracle(engine, oracle, sc, rowptr, col, case)
    elif case == "16_runs_of_64":
        assert rp[1] == 16 and (w[:16] == 64).all()


# ---- 8. the CSR input and the dense table input on the same hits --------------------------------------------------
def test_csr_and_dense_table_build_the_same_graph(engine, synth, oracle):
    sc = _real_scene(synth)
    k, r = 17, REAL_RADIUS[17]
    table = _hit_table(sc.src, sc.dst, k, r)
    assert 0 < (table < 0).sum() < table.size
    engine.set_correspondences(sc.src, sc.dst)
    engine.build_neighbors_knn(k, radius=r)                            # dense n x k table with -1 entries
    dense = engine.get_sym_graph()
    rowptr, col = _csr_of_table(table)                                 # the same hits, the cut ones simply absent
    engine.set_neighbors_csr(rowptr, col)
    csr = engine.get_sym_graph()
    _assert_graph(csr, dense, "CSR input against dense table input")
    _assert_graph(csr, oracle.build_sym_graph(sc.n, rowptr, col), "CSR input against the reference")


# ---- 9. site counts around the scan and tile widths ----------------------------------------------------------------
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2048, 4097])
def test_knn_site_counts_around_the_scan_width(engine, oracle, n):
    """k_scan and k_grid_scan work 1024 wide, k_knn and k_radius in tiles of 256: a count on, below and above each."""
    src, dst = _exact_scene(n, seed=200 + n)
    engine.set_correspondences(src, dst)
    _check_knn(engine, oracle, src, dst, 16, exact=True)
    r = 60.0
    D, _ = _exact_distances(src, dst)
    hit = D <= int(np.float32(r) * np.float32(r))
    rowptr = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.int32)
    col = np.nonzero(hit)[1].astype(np.int32)
    assert col.size > n
    assert engine.build_neighbors_radius(r) == col.size
    _assert_graph(engine.get_sym_graph(), oracle.build_sym_graph(n, rowptr, col), f"radius builder n={n}")
