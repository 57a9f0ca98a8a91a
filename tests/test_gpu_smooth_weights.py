"""The distance-weighted smoothness on the GPU (include/multih_hip.h, mh_set_smoothness_weights; csrc/graph.hip, k_arc_weights):
the weights and the multiplicities against the numpy twin (tests/smooth_weights_numpy.py) on graphs at the kernel's edges, the
engine's state around the setting, and everything that reads the weights — mh_expand (against the reference's GCO and the oracle on
the repeated-hit list, so the per-site totals of the dominance reduction are held too), mh_labeling_step, mh_labeling_energy,
mh_merge_deltas, mh_drop_deltas, and Process() through the host class.  Every comparison is in exact integers."""
import ctypes as C
import os

import numpy as np
import pytest

import data_term_numpy as T
import expand_tables as X
import label_cost_numpy as L
import merge_energy_numpy as M
import smooth_weights_numpy as S

pytestmark = pytest.mark.gpu

INVALID, NOT_SET, OVERFLOW = -2, -4, -5
LAM, THR, THR2, LOCALITY = 0.5, 2.2, 2.2 ** 2, 0.005
POTTS = 50                                                  # round(100 * LAM)


@pytest.fixture
def restore(engine):
    yield
    for k, v in X.SCHEDULE_DEFAULTS.items():
        engine.set_tuning(k, v)


def _code(mh, fn):
    with pytest.raises(mh.MultiHError) as ei:
        fn()
    return ei.value.code


def _points(rng, n, extent=300.0):
    return np.ascontiguousarray(rng.uniform(0, extent, size=(n, 2))), np.ascontiguousarray(rng.uniform(0, extent, size=(n, 2)))


def _load_table(e, src, dst, cost):
    """X.load_into_engine with real correspondences and without the graph: the cost buffer sized by mh_data_cost over L - 1 dummy
    models, then overwritten with `cost`."""
    n, Lc = cost.shape
    e.set_params(3.0, 2.5, 0.002, LAM, 0)
    e.set_correspondences(src, dst)
    e.set_models(np.tile(np.eye(3).reshape(1, 9), (Lc - 1, 1)))
    e.data_cost(fetch=False)
    ptr, nbytes = e.device_buffer(X.MH_BUF_COST)
    assert nbytes >= 4 * n * Lc
    e.synchronize()
    c = np.ascontiguousarray(cost, dtype=np.int32)
    assert X._hip_runtime().hipMemcpy(C.c_void_p(ptr), c.ctypes.data_as(C.c_void_p), 4 * n * Lc, 1) == 0


def _graph_in_force(engine, oracle, src, dst, hits, rule, rho, q_max):
    """The engine's graph against the oracle's folding of the hits and the twin's weights; returns (rowptr, col, mult, w)."""
    n = src.shape[0]
    rp, cl, w = engine.get_sym_graph()
    mult = engine.sym_multiplicity()
    rp_o, cl_o, mult_o = oracle.build_sym_graph(n, *hits)
    assert np.array_equal(rp, rp_o) and np.array_equal(cl, cl_o)
    assert np.array_equal(mult, mult_o)
    want = S.arc_weights(src, dst, rp, cl, mult, rule, rho, q_max)
    assert np.array_equal(w.astype(np.int64), want), np.flatnonzero(w != want)[:10]
    return rp, cl, mult, want


def _expand_against_oracle(engine, oracle, cost, rp, cl, w, reference=False, init=None):
    """mh_expand on the table the engine holds against the oracle (labels, energy, cycles) on the repeated-hit list — the
    dominance reduction in front of the solver reads the per-site totals —, and against the reference's GCO where asked."""
    wrp, wcol = S.weighted_hits(rp, cl, w)
    p = X.Problem("weighted", cost, wrp, wcol, POTTS, init)
    lab_o, e_o, cyc_o, _ = oracle.expand(cost, wrp, wcol, POTTS, init_labels=init)
    if reference:
        assert X.gco_neighbour_entries_fit(p)
        if oracle.ref() is not None:      # (where oracle/_ref is not built the oracle stands in: the CPU suite holds the two equal on these graphs)
            lab_r, e_r = oracle.ref_expand_table(cost, wrp, wcol, POTTS, init_labels=init)
            assert e_r == e_o and np.array_equal(lab_r, lab_o)
    lab, e, cyc = engine.expand(init)
    assert e == e_o and cyc == cyc_o
    assert np.array_equal(lab, lab_o), int((lab != lab_o).sum())
    assert X.energy_np(cost, wrp, wcol, POTTS, lab) == e
    return lab, e


def _edge_graph_cases():
    """(name, src, dst, (hit_rowptr, hit_col)) at the edges of the row kernels."""
    out = []
    rng = np.random.default_rng(5)
    # duplicates, self hits and hits both ways
    n = 300
    src, dst = _points(rng, n)
    out.append(("multi", src, dst, X.graph_random_multi(n, rng, deg=5)))
    # rows of 0, 1, 15, 16, 17 entries: centres with that many leaves each, and an isolated site
    rows, cols, nxt = [], [], 5
    for c, r in enumerate((1, 15, 16, 17)):
        rows += [c] * r
        cols += list(range(nxt, nxt + r))
        nxt += r
    n = nxt
    src, dst = _points(rng, n, 60.0)
    out.append(("lane-edges", src, dst, X.csr(n, rows, cols)))
    # a hub whose raw row has 1023, 1024 (the device's fold) and 1025 entries (the host fallback)
    for m in (1023, 1024, 1025):
        n = 1100
        src, dst = _points(rng, n, 120.0)
        others = np.arange(1, m + 1)
        ring = np.arange(1, n - 1)
        out.append((f"hub-{m}", src, dst, X.csr(n, np.concatenate([others, ring]), np.concatenate([np.zeros(m, np.int64), ring + 1]))))
    # coincident points: d == 0 on many arcs
    n = 200
    src, dst = _points(rng, n)
    src[:120], dst[:120] = src[0], dst[0]
    src[120:160], dst[120:160] = src[120], dst[120]
    out.append(("coincident", src, dst, X.graph_random_multi(n, rng, deg=4)))
    # float32 distances that overflow (infinite) and coordinates beyond float32 (inf - inf: NaN)
    n = 64
    src, dst = _points(rng, n)
    src[:8, 0] = [3e19, -3e19, 2.5e19, -2.5e19, 1e300, 1e300, -1e300, 3e38]
    dst[8:12, 1] = [1e25, -1e25, 1e300, 1e300]
    out.append(("overflow", src, dst, X.csr(n, np.repeat(np.arange(n), 3), (np.repeat(np.arange(n), 3) + np.tile([1, 2, 5], n)) % n)))
    # n == 1 (no arc at all, a self hit) and n == 2
    out.append(("n1", np.array([[1.0, 2.0]]), np.array([[3.0, 4.0]]), (np.array([0, 1], np.int32), np.array([0], np.int32))))
    out.append(("n2", np.array([[1.0, 2.0], [4.0, 6.0]]), np.array([[3.0, 4.0], [3.0, 16.0]]),
                (np.array([0, 2, 3], np.int32), np.array([1, 1, 0], np.int32))))
    return out


EDGE_CASES = _edge_graph_cases()


# ---- 1. the kernel against the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_weights_on_edge_graphs(engine, oracle, case):
    name, src, dst, hits = case
    n = src.shape[0]
    rng = np.random.default_rng(n)
    cost = X.costs_outlier_per_site(rng, n, 4)
    rho, q_max = (40.0, 8) if name != "n2" else (13.0, 256)
    with np.errstate(all="ignore"):
        _load_table(engine, src, dst, cost)
        engine.set_neighbors_csr(*hits)
        rp, cl, mult, w = _graph_in_force(engine, oracle, src, dst, hits, S.UNIFORM, 0.0, 1)
        engine.set_smoothness_weights("cauchy", rho, q_max)
        rp, cl, mult, w = _graph_in_force(engine, oracle, src, dst, hits, S.CAUCHY, rho, q_max)
    if name == "lane-edges":
        assert sorted(set(np.diff(rp).tolist())) == [0, 1, 15, 16, 17]
    if name.startswith("hub"):
        assert np.diff(rp)[0] == int(name[4:]) and (w[:rp[1]] > mult[:rp[1]]).any()
    if name == "coincident":
        assert (w == 8 * mult).sum() > 100
    if name == "overflow":
        rows = np.repeat(np.arange(n), np.diff(rp))
        far = (rows < 12) | (cl < 12)                     # an end among the sites with the huge coordinates
        assert far.sum() >= 60 and (w[far] == mult[far]).all()
    if name == "n2":
        # d = (9 + 16) + 0 + 144 = 169 = rho^2: t = 1/2, q = 128; three hits between the two sites
        assert rp.tolist() == [0, 1, 2] and mult.tolist() == [3, 3] and w.tolist() == [384, 384]
    if name == "n1":
        assert rp.tolist() == [0, 0] and w.size == 0
    _expand_against_oracle(engine, oracle, cost, rp, cl, w)


# ---- 2. state -----------------------------------------------------------------------------------------------------------------
def test_setting_is_sticky_and_applies_to_resident_and_later_graphs(mh, engine, oracle):
    src, dst, H = S.two_planes(600, 3)
    hits = S.knn_hits(src, dst, 6)
    src2, dst2, _ = S.two_planes(700, 4)
    hits2 = S.knn_hits(src2, dst2, 6)
    engine.set_correspondences(src, dst)
    # before any graph: remembered
    engine.set_smoothness_weights("cauchy", 40.0, 8)
    assert _code(mh, engine.get_sym_graph) == NOT_SET and _code(mh, engine.sym_multiplicity) == NOT_SET
    engine.build_neighbors_knn(6)
    rp, cl, mult, w_before = _graph_in_force(engine, oracle, src, dst, hits, S.CAUCHY, 40.0, 8)
    assert set(np.unique(w_before // mult).tolist()) == set(range(1, 9))
    # back to uniform: the multiplicities, no rebuild; and after the build: the same weights as before it
    engine.set_smoothness_weights("uniform")
    _graph_in_force(engine, oracle, src, dst, hits, S.UNIFORM, 0.0, 1)
    engine.set_smoothness_weights(S.UNIFORM, float("nan"), -7)                  # rho and q_max are not looked at
    engine.set_smoothness_weights("cauchy", 40.0, 8)
    _, _, _, w_after = _graph_in_force(engine, oracle, src, dst, hits, S.CAUCHY, 40.0, 8)
    assert np.array_equal(w_after, w_before)
    # q_max == 1 is the uniform graph; another rho and q_max replace the weights
    engine.set_smoothness_weights("cauchy", 40.0, 1)
    _, _, m1, w1 = _graph_in_force(engine, oracle, src, dst, hits, S.CAUCHY, 40.0, 1)
    assert np.array_equal(w1, m1)
    engine.set_smoothness_weights("cauchy", 7.5, 256)
    _graph_in_force(engine, oracle, src, dst, hits, S.CAUCHY, 7.5, 256)
    # every way a graph arrives picks the setting up
    engine.set_neighbors_csr(*hits)
    _graph_in_force(engine, oracle, src, dst, hits, S.CAUCHY, 7.5, 256)
    engine.build_neighbors_knn(6, radius=1e6)
    _graph_in_force(engine, oracle, src, dst, hits, S.CAUCHY, 7.5, 256)
    # a new point set drops the graph, not the setting
    engine.set_correspondences(src2, dst2)
    assert _code(mh, engine.get_sym_graph) == NOT_SET
    engine.build_neighbors_knn(6)
    _graph_in_force(engine, oracle, src2, dst2, hits2, S.CAUCHY, 7.5, 256)
    # invalid arguments change nothing
    bad = [(2, 40.0, 8), (-1, 40.0, 8), (1, 0.0, 8), (1, -1.0, 8), (1, float("nan"), 8), (1, float("inf"), 8), (1, 40.0, 0),
           (1, 40.0, 257), (1, 40.0, -3)]
    for rule, rho, q in bad:
        assert engine.lib.mh_set_smoothness_weights(engine._h, rule, C.c_double(rho), q) == INVALID, (rule, rho, q)
    assert engine.lib.mh_set_smoothness_weights(None, 1, C.c_double(40.0), 8) == INVALID
    with pytest.raises(ValueError):
        engine.set_smoothness_weights("gauss", 40.0, 8)
    _graph_in_force(engine, oracle, src2, dst2, hits2, S.CAUCHY, 7.5, 256)


def test_host_fallback_graph_returns_the_weights_in_force(engine, oracle):
    """A raw row of more than 1024 entries is folded on the host, which leaves a host copy of the MULTIPLICITIES: mh_get_sym_graph
    must hand out the weights in force all the same — set before the build, after it, and after the read-out."""
    name, src, dst, hits = [c for c in EDGE_CASES if c[0] == "hub-1025"][0]
    engine.set_correspondences(src, dst)
    engine.set_smoothness_weights("cauchy", 60.0, 16)
    engine.set_neighbors_csr(*hits)
    _, _, mult, w = _graph_in_force(engine, oracle, src, dst, hits, S.CAUCHY, 60.0, 16)
    assert (w != mult).sum() > 1000
    engine.set_smoothness_weights("uniform")
    _graph_in_force(engine, oracle, src, dst, hits, S.UNIFORM, 0.0, 1)
    engine.set_neighbors_csr(*hits)
    _graph_in_force(engine, oracle, src, dst, hits, S.UNIFORM, 0.0, 1)
    engine.set_smoothness_weights("cauchy", 25.0, 5)
    _graph_in_force(engine, oracle, src, dst, hits, S.CAUCHY, 25.0, 5)


def test_overflow_leaves_the_weights_in_force(mh, engine, oracle):
    """mult * q beyond int32: n = 2, one hit repeated 2^23 + 1 times, coincident sites (q = q_max = 256)."""
    reps = (1 << 23) + 1
    src, dst = np.array([[5.0, 6.0], [5.0, 6.0]]), np.array([[7.0, 8.0], [7.0, 8.0]])
    hits = (np.array([0, reps, reps], np.int32), np.zeros(reps, np.int32) + 1)
    engine.set_correspondences(src, dst)
    engine.set_neighbors_csr(*hits)
    rp, cl, w = engine.get_sym_graph()
    assert rp.tolist() == [0, 1, 2] and cl.tolist() == [1, 0] and w.tolist() == [reps, reps]
    assert _code(mh, lambda: engine.set_smoothness_weights("cauchy", 40.0, 256)) == OVERFLOW
    assert engine.get_sym_graph()[2].tolist() == [reps, reps] and engine.sym_multiplicity().tolist() == [reps, reps]
    engine.set_smoothness_weights("cauchy", 40.0, 255)                       # (2^23 + 1) * 255 < 2^31
    assert engine.get_sym_graph()[2].tolist() == [255 * reps, 255 * reps]
    assert _code(mh, lambda: engine.set_smoothness_weights("cauchy", 40.0, 256)) == OVERFLOW
    assert engine.get_sym_graph()[2].tolist() == [255 * reps, 255 * reps] and engine.sym_multiplicity().tolist() == [reps, reps]
    engine.set_smoothness_weights("uniform")
    assert engine.get_sym_graph()[2].tolist() == [reps, reps]


def test_row_sum_overflow_is_refused(mh, engine):
    half = (1 << 22) + 1
    src, dst = np.zeros((3, 2)), np.zeros((3, 2))
    hits = (np.array([0, 2 * half, 2 * half, 2 * half], np.int32), np.concatenate([np.full(half, 1), np.full(half, 2)]).astype(np.int32))
    engine.set_correspondences(src, dst)
    engine.set_neighbors_csr(*hits)
    assert engine.get_sym_graph()[2].tolist() == [half, half, half, half]
    assert 256 * half <= X.INT32_MAX < 2 * 256 * half                    # each product fits, the hub's total does not
    assert _code(mh, lambda: engine.set_smoothness_weights("cauchy", 1.0, 256)) == OVERFLOW
    assert engine.get_sym_graph()[2].tolist() == [half, half, half, half]
    engine.set_smoothness_weights("cauchy", 1.0, 255)
    assert engine.get_sym_graph()[2].tolist() == [255 * half] * 4
    # a graph that arrives under a rule it overflows is refused, and the engine then holds none
    engine.set_correspondences(src, dst)
    engine.set_smoothness_weights("cauchy", 1.0, 256)
    assert _code(mh, lambda: engine.set_neighbors_csr(*hits)) == OVERFLOW
    assert _code(mh, engine.get_sym_graph) == NOT_SET
    engine.set_smoothness_weights("cauchy", 1.0, 255)
    engine.set_neighbors_csr(*hits)
    assert engine.get_sym_graph()[2].tolist() == [255 * half] * 4


# ---- 3. mh_expand against the reference's GCO -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,q_max,labels", [(600, 6, 8, 5), (2000, 8, 16, 17)])
def test_expand_equals_reference_gco_on_a_real_data_cost(engine, oracle, restore, n, k, q_max, labels):
    src, dst, H = S.two_planes(n, 3)
    rng = np.random.default_rng(n)
    while H.shape[0] < labels - 1:
        H = np.concatenate([H, H[rng.integers(0, 2)][None] * (1 + 3e-4 * rng.normal(size=(1, 9)))])
    hits = S.knn_hits(src, dst, k)
    engine.set_correspondences(src, dst)
    engine.set_models(H)
    engine.set_smoothness_weights("cauchy", 40.0, q_max)
    engine.build_neighbors_knn(k)
    rp, cl, mult, w = _graph_in_force(engine, oracle, src, dst, hits, S.CAUCHY, 40.0, q_max)
    cost = engine.data_cost()
    assert cost.shape == (n, labels) and np.array_equal(cost, oracle.data_cost(src, dst, H, LAM, THR2))
    lab_u = oracle.expand(cost, *hits, POTTS)[0]
    for sched in [{}] + X.class_s_schedules(n, 2, n):
        for key, v in X.SCHEDULE_DEFAULTS.items():
            engine.set_tuning(key, sched.get(key, v))
        lab, e = _expand_against_oracle(engine, oracle, cost, rp, cl, w, reference=True)
        assert engine.expand_stats()["barrier_timeout_retries"] == 0
    assert not np.array_equal(lab, lab_u), "the weights should change the labeling"


# ---- 4. mh_labeling_step --------------------------------------------------------------------------------------------------------
def test_labeling_step_cold_and_warm(engine, synth, oracle):
    sc = synth.make_scene(1000, 3, seed=2, knn=8, symmetric=False)
    hits = (sc.hit_rowptr, sc.hit_col)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_epipolar(sc.F, sc.e2)
    engine.set_neighbors_csr(*hits)
    engine.set_smoothness_weights("cauchy", 60.0, 8)
    rp, cl, mult, w = _graph_in_force(engine, oracle, sc.src, sc.dst, hits, S.CAUCHY, 60.0, 8)
    assert len(np.unique(w // mult)) >= 4
    wrp, wcol = S.weighted_hits(rp, cl, w)
    H = sc.H_true * (1.0 + np.random.default_rng(2).normal(0, 1e-4, size=sc.H_true.shape))
    engine.set_models(H)
    lab = np.full(sc.n, -1, dtype=np.int32)
    lab_ref, H_ref = lab.copy(), H.copy()
    uniform = oracle.labeling_step(sc.src, sc.dst, sc.aff, H, LAM, THR2, *hits, False, sc.F, sc.e2, lab)
    for it in range(3):
        warm = it > 0
        lab, energy, cycles = engine.labeling_step(warm, lab)
        lab_ref, H_ref, e_ref, cyc_ref = oracle.labeling_step(sc.src, sc.dst, sc.aff, H_ref, LAM, THR2, wrp, wcol, warm, sc.F, sc.e2, lab_ref)
        assert energy == e_ref and cycles == cyc_ref, it
        assert np.array_equal(lab, lab_ref), it
        if it == 0:
            assert e_ref != uniform[2]
        Hg = engine.get_models()
        scale = np.max(np.abs(H_ref), axis=1, keepdims=True)
        assert np.max(np.abs(Hg - H_ref) / scale) <= 1e-6
        assert np.array_equal(Hg.view(np.uint64), H_ref.view(np.uint64)), it


# ---- 5. energy and deltas -------------------------------------------------------------------------------------------------------
def test_energy_merge_and_drop_deltas_read_the_weights_in_force(engine, synth, oracle):
    sc = synth.make_scene(1200, 3, seed=9, knn=6, symmetric=False)
    src, dst = sc.src, sc.dst
    rng = np.random.default_rng(9)
    H = np.ascontiguousarray(np.concatenate([sc.H_true, sc.H_true[:1] * (1 + 1e-4 * rng.normal(size=(1, 9)))]))      # label 3 splits plane 0
    labels = sc.gt_label.astype(np.int32).copy()
    half = (labels == 0) & (rng.random(sc.n) < 0.5)
    labels[half] = 3
    flip = rng.random(sc.n) < 0.05
    labels[flip] = rng.integers(-1, 4, size=int(flip.sum()))
    hits = (sc.hit_rowptr, sc.hit_col)
    engine.set_correspondences(src, dst)
    engine.set_neighbors_csr(*hits)
    engine.set_models(H)
    uniform_energy = engine.labeling_energy(labels)
    engine.data_cost(fetch=False)
    engine.set_smoothness_weights("cauchy", 60.0, 8)
    rp, cl, mult, w = _graph_in_force(engine, oracle, src, dst, hits, S.CAUCHY, 60.0, 8)
    g = (rp, cl, w)
    before = engine.labeling_energy(labels)
    assert before == M.labeling_energy(src, dst, labels, H, *g, LAM, THR2, T.REFERENCE, False)
    assert before[1] == uniform_energy[1] and before[2] > uniform_energy[2]
    # the data cost (computed under the uniform rule) did not go stale, and mh_expand's energy of its own labeling is mh_labeling_energy's
    lab, energy, _ = engine.expand()
    assert engine.labeling_energy(lab - 1)[0] == energy
    pairs = np.array([(a, b) for a in range(4) for b in range(a + 1, 4)], dtype=np.int32)
    Hs, delta, parts, status = engine.merge_deltas(labels, pairs)
    want_H, want_delta, want_parts, want_status = M.merge_deltas(src, dst, labels, H, pairs, *g, LAM, THR2, T.REFERENCE, False)
    assert np.array_equal(status, want_status) and (status == M.OK).all()
    assert np.array_equal(delta, want_delta) and np.array_equal(parts, want_parts)
    for k in range(len(pairs)):
        lab2, H2 = M.apply_merges(labels, H, pairs, Hs, [k])
        engine.set_models(H2)
        after = engine.labeling_energy(lab2)
        assert after[0] - before[0] == delta[k] and after[2] - before[2] == -parts[k, 3], (pairs[k], after, before, delta[k])
    engine.set_models(H)
    cand = np.arange(4, dtype=np.int32)
    d_delta, d_parts, d_status, alt = engine.drop_deltas(labels, cand)
    w_delta, w_parts, w_status, _ = L.drop_deltas(src, dst, labels, H, cand, *g, LAM, THR2, T.REFERENCE, False)
    assert np.array_equal(d_status, w_status) and (d_status == L.OK).all()
    assert np.array_equal(d_delta, w_delta) and np.array_equal(d_parts, w_parts)
    for k in range(4):
        after = engine.labeling_energy(L.labels_after_drop(labels, k, alt))
        assert after[0] - before[0] == d_delta[k], (k, after, before, d_delta[k])
        assert after[2] - before[2] == d_parts[k, 4] - d_parts[k, 3]


# ---- 6. Process() through the host class -------------------------------------------------------------------------------------------
def _host(mh):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_smoothness_weights.argtypes = [C.c_int, C.c_double, C.c_int]
    host.mhh_set_smoothness_weights.restype = None
    return host


def _run_process(host, sc, seed, H0, smoothness=None, hits=None):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((256, 9))
    it, en = C.c_int(-1), C.c_double(-1)
    src, dst, aff, F, e2, H0 = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff, sc.F, sc.e2, H0))
    host.mhh_set_post_filter(0)
    if smoothness is not None:
        host.mhh_set_smoothness_weights(*smoothness)
    if hits is not None:
        rp, col = (np.ascontiguousarray(a, dtype=np.int32) for a in hits)
        host.mhh_set_neighbour_hits(rp.ctypes.data_as(ip), col.ctypes.data_as(ip), sc.n)
    try:
        k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, F.ctypes.data_as(dp),
                                 e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(THR), C.c_double(LOCALITY), C.c_double(LAM), 20,
                                 C.c_ulonglong(seed), 0, 0, 0, H0.ctypes.data_as(dp), H0.shape[0], labels.ctypes.data_as(ip),
                                 Hout.ctypes.data_as(dp), 256, C.byref(it), C.byref(en), None, 0, 4)
    finally:
        host.mhh_set_post_filter(1)
        host.mhh_set_smoothness_weights(-1, 0.0, 16)
        host.mhh_set_neighbour_hits(None, None, 0)
    return k, labels, Hout[:max(k, 0)].copy(), it.value, en.value


def _initial_models(sc, seed):
    rng = np.random.default_rng(seed)
    extra = sc.H_true[rng.integers(0, sc.H_true.shape[0], size=2)] * (1.0 + rng.normal(0, 2e-4, size=(2, 9)))
    return np.ascontiguousarray(np.concatenate([sc.H_true * (1.0 + rng.normal(0, 1e-4, size=sc.H_true.shape)), extra]))


def test_process_with_q_max_1_is_the_default_run(mh, engine_lib, synth):
    sc = synth.make_scene(1000, 3, seed=2, with_neighbours=False)
    host, H0 = _host(mh), _initial_models(sc, 2)
    k, labels, H, it, en = _run_process(host, sc, 2, H0)
    assert k >= 2 and it >= 1
    for smoothness in ((S.CAUCHY, 40.0, 1), (S.UNIFORM, 0.0, 0)):
        k2, labels2, H2, it2, en2 = _run_process(host, sc, 2, H0, smoothness)
        assert (k2, it2, en2) == (k, it, en) and np.array_equal(labels2, labels)
        assert np.array_equal(H2.view(np.uint64), H.view(np.uint64))
    # and a setting the class refuses makes Process() fail
    assert _run_process(host, sc, 2, H0, (S.CAUCHY, 0.0, 8))[0] == -1
    assert _run_process(host, sc, 2, H0, (S.CAUCHY, 40.0, 257))[0] == -1
    assert _run_process(host, sc, 2, H0, (7, 40.0, 8))[0] == -1


def test_process_with_explicit_neighbours_equals_the_oracle(mh, engine_lib, synth, oracle):
    sc = synth.make_scene(1000, 3, seed=7, knn=8, symmetric=False)
    hits = (sc.hit_rowptr, sc.hit_col)
    host, H0 = _host(mh), _initial_models(sc, 7)
    rp, cl, mult = oracle.build_sym_graph(sc.n, *hits)
    w = S.arc_weights(sc.src, sc.dst, rp, cl, mult, S.CAUCHY, 60.0, 8)
    assert len(np.unique(w // mult)) >= 4
    wrp, wcol = S.weighted_hits(rp, cl, w)
    assert X.gco_neighbour_entries_fit(X.Problem("process", np.zeros((sc.n, 1), np.int32), wrp, wcol, POTTS))
    want = oracle.process(sc.src, sc.dst, sc.aff, sc.F, sc.e2, THR, LOCALITY, LAM, 20, 7, wrp, wcol, init_H=H0, post_filter=False)
    uniform = oracle.process(sc.src, sc.dst, sc.aff, sc.F, sc.e2, THR, LOCALITY, LAM, 20, 7, *hits, init_H=H0, post_filter=False)
    assert want["energy"] != uniform["energy"]
    k, labels, H, it, en = _run_process(host, sc, 7, H0, (S.CAUCHY, 60.0, 8), hits)
    assert k == want["H"].shape[0] and it == want["iterations"] and en == want["energy"]
    assert np.array_equal(labels, want["labels"]), int((labels != want["labels"]).sum())
    scale = np.max(np.abs(want["H"]), axis=1, keepdims=True)
    assert np.max(np.abs(H - want["H"]) / scale) <= 1e-9


def test_known_answer_where_the_weights_change_the_labeling(engine, oracle):
    """Five sites on a line, neighbours in a chain; sites 0-2 lie 1 px apart, site 3 is 100 px from site 2, site 4 one px further.
    Only label 1 suits the left end (site 0: 10 against 300), label 2 is free everywhere else and label 1 costs 40 at sites 1, 2 and 90
    at sites 3, 4.  Uniform weights (Potts 50 an arc) let site 0 stand alone: 10 + 50 for the cut 0|1.  Under CAUCHY(rho 10, q_max 8)
    the near arcs weigh 8 and the long arc 1, so the cut 0|1 costs 400: the cut moves to the long arc (50) and sites 1, 2 pay 40 each
    for label 1 — 140, against 410 for the uniform answer, 300 for label 2 everywhere and 270 for label 1 everywhere."""
    x = np.array([0.0, 1.0, 2.0, 102.0, 103.0])
    src = np.ascontiguousarray(np.stack([x, np.zeros(5)], axis=1))
    dst = src.copy()
    hits = X.graph_path(5)
    cost = np.array([[500, 10, 300], [500, 40, 0], [500, 40, 0], [500, 90, 0], [500, 90, 0]], dtype=np.int32)
    assert len(cost) <= 12 and cost.shape[1] <= 4                               # X.tiny_problems' sizes: the brute force applies
    _load_table(engine, src, dst, cost)
    engine.set_neighbors_csr(*hits)
    rp, cl, mult, w = _graph_in_force(engine, oracle, src, dst, hits, S.UNIFORM, 0.0, 1)
    lab_u, e_u = _expand_against_oracle(engine, oracle, cost, rp, cl, w, reference=True)
    assert lab_u.tolist() == [1, 2, 2, 2, 2] and e_u == 10 + 50
    engine.set_smoothness_weights("cauchy", 10.0, 8)
    rp, cl, mult, w = _graph_in_force(engine, oracle, src, dst, hits, S.CAUCHY, 10.0, 8)
    # d = 2 (both images move): q = round(8 * 100 / 102) = 8; d = 20000: 8 * 100 / 20100 < 1 -> 1
    assert w.tolist() == [8, 8, 8, 8, 1, 1, 8, 8]
    wrp, wcol = S.weighted_hits(rp, cl, w)
    assert X.gco_neighbour_entries_fit(X.Problem("tiny", cost, wrp, wcol, POTTS)) is False      # 16 entries at 5 sites: the oracle, not GCO
    lab_w, e_w = _expand_against_oracle(engine, oracle, cost, rp, cl, w)
    assert lab_w.tolist() == [1, 1, 1, 2, 2] and e_w == 10 + 40 + 40 + 50
    for lab, e, (hr, hc) in ((lab_u, e_u, hits), (lab_w, e_w, (wrp, wcol))):
        best, alpha = X.best_expansion_move(cost, hr, hc, POTTS, lab)
        assert best == e and alpha == -1
    assert X.energy_int(cost, wrp, wcol, POTTS, lab_u) == 10 + 400 > e_w
