"""GPU parity tests proper: every kernel called through the C ABI and compared
with the CPU oracle on the same seeded inputs.  Integer results (counts, costs,
labels, energies, sample indices) must be bit-exact; FP64 results of the
reference's formulas (residuals) must be bit-exact too, because both sides
round every operation once in the reference's order; homographies must agree
to 1e-6 relative (north_star) — in practice they are bit-identical."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = 2.2
THR2 = THR * THR
LAM = 0.5


def _load(engine, sc, neighbours=True):
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.set_epipolar(sc.F, sc.e2)
    if neighbours:
        engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)


def _models(sc, rng, extra=5):
    """Ground-truth planes plus perturbed copies (near-miss models make interesting costs)."""
    H = [sc.H_true]
    for _ in range(extra):
        k = rng.integers(0, sc.H_true.shape[0])
        H.append(sc.H_true[k:k + 1] * (1.0 + rng.normal(0, 2e-4, size=(1, 9))))
    return np.concatenate(H, axis=0)


@pytest.mark.parametrize("n,k,seed", [(1, 1, 5), (2, 1, 6), (129, 2, 1), (1000, 3, 2), (5000, 3, 1234), (4099, 4, 7)])
def test_residual_matrix_and_counts_bit_exact(engine, synth, oracle, n, k, seed):
    sc = synth.make_scene(n, k, seed=seed, with_neighbours=False)
    rng = np.random.default_rng(seed)
    H = _models(sc, rng, extra=17)          # 17+k models: exercises the partial last model chunk
    _load(engine, sc, neighbours=False)
    engine.set_models(H)
    R, cnt = engine.residual_matrix(THR2)
    R_ref = oracle.residual_matrix(sc.src, sc.dst, H)
    assert R.shape == R_ref.shape
    assert np.array_equal(R.view(np.uint64), R_ref.view(np.uint64)), "residuals differ in the last bit somewhere"
    assert np.array_equal(cnt, oracle.score(sc.src, sc.dst, H, THR2))
    # fused score kernel (no matrix) gives the same counts
    assert np.array_equal(engine.score(THR2), cnt)


def test_residual_nonfinite_and_degenerate_models(engine, synth, oracle):
    """Degenerate hypotheses (s == 0, huge/denormal scale) must round identically: inf/NaN
    patterns are compared bitwise except NaN payloads (compared as NaN-ness)."""
    sc = synth.make_scene(777, 2, seed=3, with_neighbours=False)
    H = np.array([
        [1, 0, 0, 0, 1, 0, 0, 0, 0],            # s == 0 everywhere -> inf/NaN
        [1, 0, 0, 0, 1, 0, 1e-3, -1e-3, 0],      # s crosses zero
        [1e-300, 0, 0, 0, 1e-300, 0, 0, 0, 1e-300],   # tiny scale
        [1e150, 0, 0, 0, 1e150, 0, 0, 0, 1e150],      # huge scale
        [0, 0, 0, 0, 0, 0, 0, 0, 1],
    ], dtype=np.float64)
    _load(engine, sc, neighbours=False)
    engine.set_models(H)
    with np.errstate(all="ignore"):
        R, cnt = engine.residual_matrix(THR2)
        R_ref = oracle.residual_matrix(sc.src, sc.dst, H)
    nan = np.isnan(R_ref)
    assert np.array_equal(np.isnan(R), nan)
    assert np.array_equal(R[~nan].view(np.uint64), R_ref[~nan].view(np.uint64))
    assert np.array_equal(cnt, oracle.score(sc.src, sc.dst, H, THR2))


def test_score_with_point_mask(engine, synth, oracle):
    sc = synth.make_scene(3001, 3, seed=11, with_neighbours=False)
    rng = np.random.default_rng(0)
    H = _models(sc, rng, extra=30)
    mask = (rng.random(sc.n) < 0.6).astype(np.uint8)
    _load(engine, sc, neighbours=False)
    engine.set_models(H)
    assert np.array_equal(engine.score(THR2, mask=mask), oracle.score(sc.src, sc.dst, H, THR2, mask=mask))
    assert np.array_equal(engine.score(THR2, mask=np.zeros(sc.n, np.uint8)), np.zeros(H.shape[0], np.int32))


def test_inliers_of_model(engine, synth, oracle):
    sc = synth.make_scene(2000, 3, seed=4, with_neighbours=False)
    _load(engine, sc, neighbours=False)
    engine.set_models(sc.H_true)
    lab0 = np.full(sc.n, -1, dtype=np.int32)
    got = engine.inliers_of_model(1, THR2, 0, lab0)
    d2 = oracle.residual_matrix(sc.src, sc.dst, sc.H_true[1:2])[0]
    assert np.array_equal(got, np.where(d2 < THR2, 0, -1))


@pytest.mark.parametrize("n,k,seed", [(64, 3, 1), (1000, 3, 2), (5000, 10, 3)])
def test_data_cost_bit_exact(engine, synth, oracle, n, k, seed):
    sc = synth.make_scene(n, k, seed=seed, with_neighbours=False)
    H = _models(sc, np.random.default_rng(seed))
    _load(engine, sc, neighbours=False)
    engine.set_models(H)
    cost = engine.data_cost()
    assert np.array_equal(cost, oracle.data_cost(sc.src, sc.dst, H, LAM, THR2))
    # known-answer constants of the harness defaults
    assert (cost[:, 0] == 4901).all()
    assert set(np.unique(cost[:, 1:])).issubset(set(range(0, 201)) | {9802})


@pytest.mark.parametrize("n,m,seed", [(50, 64, 1), (5000, 1000, 1234), (777, 333, 9)])
def test_sampling_and_dlt4(engine, synth, oracle, n, m, seed):
    sc = synth.make_scene(n, 3, seed=seed, with_neighbours=False)
    _load(engine, sc, neighbours=False)
    engine.propose_dlt4(seed, 10, m)
    idx = engine.get_samples()
    assert np.array_equal(idx, oracle.sample4(seed, 10, m, n)), "counter RNG tuples differ"
    assert all(len(set(t)) == 4 for t in idx.tolist())
    H = engine.get_models()
    H_ref, wit, _ = oracle.dlt4(sc.src, sc.dst, idx)
    good = wit > 1e-6                         # conditioning witness: skip (near-)degenerate samples
    assert good.sum() > 0.5 * m
    # north_star tolerance: 1e-6 relative (H has unit Frobenius norm, so absolute == relative)
    assert np.max(np.abs(H[good] - H_ref[good])) <= 1e-6
    # in practice both sides execute the same rounded operations
    assert np.array_equal(H[good].view(np.uint64), H_ref[good].view(np.uint64))
    # the homography maps its own 4 sample points exactly (size-independent property)
    for t in np.flatnonzero(good)[:50]:
        p = synth.apply_h(H[t], sc.src[idx[t]])
        assert np.max(np.abs(p - sc.dst[idx[t]])) < 1e-6 * 1000


def test_dlt4_register_form_equals_lds_form(engine, synth, oracle):
    """The proposer keeps W in registers and hands the columns round with DPP row shifts (dlt4.hip, k_dlt4); the
    LDS-staged form of r01-r04 is what mh_prefetch_dlt4 launches beside a resident sweep (tuning key 25 forces either).  Same rotations in the same order: every model
    bit-identical, on a scene with degenerate samples among them, and both equal to the oracle."""
    sc = synth.make_scene(300, 2, seed=21, with_neighbours=False)
    rng = np.random.default_rng(21)
    line = rng.permutation(sc.n)[:120]
    t = rng.uniform(0, 1000, size=line.size)
    sc.src[line] = np.stack([t, 0.25 * t + 50.0], axis=1)
    _load(engine, sc, neighbours=False)
    M = 8192 + 37                                  # a ragged last workgroup
    out = {}
    try:
        for form in (1, 2):
            engine.set_tuning(25, form)
            engine.propose_dlt4(77, 5, M)
            out[0 if form == 2 else 1] = (engine.get_samples().copy(), engine.get_models().copy())
    finally:
        engine.set_tuning(25, 0)
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1].view(np.uint64), out[1][1].view(np.uint64))
    with np.errstate(all="ignore"):
        H_ref, _, _ = oracle.dlt4(sc.src, sc.dst, out[0][0])
    assert np.array_equal(np.isnan(out[0][1]), np.isnan(H_ref))
    fin = ~np.isnan(H_ref).any(axis=1)
    assert np.array_equal(out[0][1][fin].view(np.uint64), H_ref[fin].view(np.uint64))


def test_dlt4_on_degenerate_samples(engine, synth, oracle):
    """Hypotheses from degenerate 4-tuples — three or four collinear points, repeated correspondences, a point set
    squeezed onto a line — are scored like any other in the bench and in Process(), so the GPU must treat them like the
    oracle: same NaN pattern in H, same bits where H is finite (both sides run the same rounded operations in the same
    order, also on a rank-deficient system), and therefore the same inlier count for EVERY hypothesis, including the
    ones whose conditioning witness is below the 1e-6 the well-conditioned test cuts at."""
    sc = synth.make_scene(400, 2, seed=13, with_neighbours=False)
    rng = np.random.default_rng(13)
    n = sc.n
    line = rng.permutation(n)[:160]                      # 40 % of the sources on one line: collinear triples and quadruples
    t = rng.uniform(0, 1000, size=line.size)
    sc.src[line] = np.stack([t, 0.5 * t + 100.0], axis=1)
    dup = rng.permutation(n)[:60]                        # repeated correspondences (distinct indices, equal coordinates)
    sc.src[dup[30:]] = sc.src[dup[:30]]
    sc.dst[dup[30:]] = sc.dst[dup[:30]]
    sc.dst[rng.permutation(n)[:40], 1] = 250.0           # some targets on a horizontal line
    _load(engine, sc, neighbours=False)
    M = 4096
    engine.propose_dlt4(5, 0, M)
    idx = engine.get_samples()
    assert np.array_equal(idx, oracle.sample4(5, 0, M, n))
    H = engine.get_models()
    with np.errstate(all="ignore"):
        H_ref, wit, _ = oracle.dlt4(sc.src, sc.dst, idx)
    bad = ~(wit > 1e-6)
    assert bad.sum() >= 50, "the scene should produce plenty of degenerate samples"
    assert np.array_equal(np.isnan(H), np.isnan(H_ref)), "NaN pattern differs"
    fin = ~np.isnan(H_ref)
    assert np.array_equal(H[fin].view(np.uint64), H_ref[fin].view(np.uint64)), \
        f"{int((H[fin].view(np.uint64) != H_ref[fin].view(np.uint64)).sum())} finite entries differ in their bits"
    cnt = engine.score(THR2)
    with np.errstate(all="ignore"):
        cnt_ref = oracle.score(sc.src, sc.dst, H_ref, THR2)
    assert np.array_equal(cnt, cnt_ref), f"counts differ for {int((cnt != cnt_ref).sum())} hypotheses"
    R, cnt_r = engine.residual_matrix(THR2)
    assert np.array_equal(cnt_r, cnt_ref)
    # four identical correspondences: the Hartley scale is 1/0, every entry of H is NaN on both sides
    sc2 = synth.make_scene(24, 1, seed=14, with_neighbours=False)
    sc2.src[:10] = sc2.src[0]
    sc2.dst[:10] = sc2.dst[0]
    _load(engine, sc2, neighbours=False)
    engine.propose_dlt4(6, 0, M)
    idx2 = engine.get_samples()
    H2 = engine.get_models()
    with np.errstate(all="ignore"):
        H2_ref, _, _ = oracle.dlt4(sc2.src, sc2.dst, idx2)
        cnt2_ref = oracle.score(sc2.src, sc2.dst, H2_ref, THR2)
    assert np.isnan(H2_ref).any(axis=1).sum() >= 20, "the scene should produce all-NaN hypotheses"
    assert np.array_equal(np.isnan(H2), np.isnan(H2_ref))
    fin2 = ~np.isnan(H2_ref)
    assert np.array_equal(H2[fin2].view(np.uint64), H2_ref[fin2].view(np.uint64))
    assert np.array_equal(engine.score(THR2), cnt2_ref)


def test_moments_and_collinearity(engine, synth, oracle):
    sc = synth.make_scene(3000, 3, seed=5, with_neighbours=False)
    H = _models(sc, np.random.default_rng(1))
    _load(engine, sc, neighbours=False)
    engine.set_models(H)
    mo, me = engine.inlier_moments(THR2)
    mo_ref, me_ref = oracle.inlier_moments(sc.src, sc.dst, H, THR2)
    assert np.array_equal(mo.view(np.uint64), mo_ref.view(np.uint64))
    assert np.array_equal(me.view(np.uint64), me_ref.view(np.uint64))     # same matrix bits, the same cyclic Jacobi


@pytest.mark.parametrize("n,k,seed", [(300, 3, 1), (5000, 3, 1234), (2000, 10, 8)])
def test_reestimate(engine, synth, oracle, n, k, seed):
    sc = synth.make_scene(n, k, seed=seed, with_neighbours=False)
    _load(engine, sc, neighbours=False)
    H0 = sc.H_true.copy()
    engine.set_models(H0)
    labels = sc.gt_label.copy()
    labels[labels == k - 1] = -1              # leave the last label empty: its H must survive untouched
    H = engine.reestimate(labels)
    H_ref, cnt = oracle.haf_reestimate(sc.src, sc.dst, sc.aff, labels, H0, sc.F, sc.e2)
    assert cnt[k - 1] == 0 and np.array_equal(H[k - 1], H0[k - 1])
    scale = np.max(np.abs(H_ref), axis=1, keepdims=True)
    assert np.max(np.abs(H - H_ref) / scale) <= 1e-6
    assert np.array_equal(H.view(np.uint64), H_ref.view(np.uint64))


@pytest.mark.parametrize("n,k,seed,sym", [(64, 2, 1, True), (300, 3, 1, True), (1000, 3, 2, False),
                                          (3000, 5, 3, True), (5000, 3, 1234, True)])
def test_expand_labels_bit_exact(engine, synth, oracle, n, k, seed, sym):
    sc = synth.make_scene(n, k, seed=seed, symmetric=sym)
    H = _models(sc, np.random.default_rng(seed), extra=3)
    _load(engine, sc)
    engine.set_models(H)
    cost = engine.data_cost()
    labels, energy, cycles = engine.expand()
    lab_ref, e_ref, cyc_ref, _ = oracle.expand(cost, sc.hit_rowptr, sc.hit_col, oracle.potts(LAM))
    assert energy == e_ref
    assert np.array_equal(labels, lab_ref)
    assert cycles == cyc_ref
    # warm start from a different labeling
    init = (sc.gt_label + 1).astype(np.int32)
    labels_w, energy_w, _ = engine.expand(init)
    lab_w_ref, e_w_ref, _, _ = oracle.expand(cost, sc.hit_rowptr, sc.hit_col, oracle.potts(LAM), init_labels=init)
    assert energy_w == e_w_ref and np.array_equal(labels_w, lab_w_ref)


@pytest.mark.parametrize("lam", [0.1, 0.5, 3.0])
def test_dominance_reduction_changes_nothing(engine, synth, oracle, lam):
    """The exact pre-solve of an alpha-move (k_reduce: sites decided by dominance, their n-links folded
    into the neighbours' t-links) must leave labels, energy and cycle count exactly as push-relabel
    alone — and as the oracle — finds them, from weak (lambda 0.1) to strong (3.0) smoothing."""
    sc = synth.make_scene(4000, 4, seed=21, noise=1.0, outlier_frac=0.3)
    H = _models(sc, np.random.default_rng(21), extra=4)
    engine.set_params(2.6, THR, 0.005, lam, 20)
    try:
        _load(engine, sc)
        engine.set_models(H)
        cost = engine.data_cost()
        lab_ref, e_ref, cyc_ref, _ = oracle.expand(cost, sc.hit_rowptr, sc.hit_col, oracle.potts(lam))
        got = {}
        # (the cascade inside the solver launch to its fixed point: with the default cap of two passes WHICH sites those
        # passes decide depends on the order the rows run in, and with it the count compared at the end)
        engine.set_tuning(17, 0)
        for rounds in (0, 1, 4):
            engine.set_tuning(6, rounds)
            labels, energy, cycles = engine.expand()
            st = engine.expand_stats()
            assert (st["reduce_launches"] > 0) == (rounds > 0)
            assert energy == e_ref and cycles == cyc_ref and np.array_equal(labels, lab_ref), f"reduce rounds {rounds}"
            got[rounds] = st
        assert got[4]["flow_moves"] <= got[0]["flow_moves"]
    finally:
        engine.set_tuning(17, 2)
        engine.set_tuning(6, 2)
        engine.set_params(2.6, THR, 0.005, LAM, 20)


def test_capped_dominance_cascade_changes_nothing(engine, synth, oracle):
    """Inside the solver launch the dominance cascade runs a bounded number of barrier-separated passes (default 2; r03) and
    ends with a pass that only folds the verdicts taken so far.  The cascade is exact but optional — what it leaves
    undecided the flow decides the same way — so labels, energy and cycles are the oracle's for every cap, on a k-NN
    graph and on a dense radius graph, cold and warm."""
    sc = synth.make_scene(4000, 4, seed=21, noise=1.0, outlier_frac=0.3)
    H = _models(sc, np.random.default_rng(21), extra=4)
    _load(engine, sc)
    engine.set_models(H)
    cost = engine.data_cost()
    lab_ref, e_ref, cyc_ref, _ = oracle.expand(cost, sc.hit_rowptr, sc.hit_col, oracle.potts(LAM))
    init = (sc.gt_label + 1).astype(np.int32)
    lab_w, e_w, cyc_w, _ = oracle.expand(cost, sc.hit_rowptr, sc.hit_col, oracle.potts(LAM), init_labels=init)
    barriers = {}
    try:
        for cap in (0, 1, 2, 3, 7):
            engine.set_tuning(17, cap)
            for grid in (256, 3):
                engine.set_tuning(5, grid)
                labels, energy, cycles = engine.expand()
                assert energy == e_ref and cycles == cyc_ref and np.array_equal(labels, lab_ref), (cap, grid)
                if grid == 256:
                    barriers[cap] = engine.expand_stats()["barriers"]
                labels, energy, cycles = engine.expand(init)
                assert energy == e_w and cycles == cyc_w and np.array_equal(labels, lab_w), (cap, grid, "warm")
    finally:
        engine.set_tuning(17, 2)
        engine.set_tuning(5, 256)
    assert barriers[2] < barriers[0], barriers


@pytest.mark.parametrize("case", ["rows_walk_several_sites", "one_workgroup", "degree_above_register_slots", "no_reduction_large_core"])
def test_expand_solver_paths(engine, synth, oracle, case):
    """The per-move solver launch (csrc/expand.hip k_solve) has several code paths that the default sizes never
    take: rows that walk several sites (core larger than the launch holds one site per row), a single workgroup,
    sites whose degree exceeds the arcs a row keeps in registers (arcs walked in memory), and the whole graph as
    core (dominance reduction off).  Each must give the oracle's labels, energy and cycle count."""
    knn = 16
    n, k, grid, reduce_rounds = 3000, 4, 256, 4
    if case == "rows_walk_several_sites":
        grid, reduce_rounds = 3, 0                       # 3 workgroups x 64 rows for ~3000 core sites
    elif case == "one_workgroup":
        grid = 1
    elif case == "degree_above_register_slots":
        knn, n = 31, 2500                                # symmetric closure of 31-NN: many sites above 48 arcs
    elif case == "no_reduction_large_core":
        n, reduce_rounds = 20000, 0                      # ~20 000 core sites > 256 workgroups x 64 rows
    sc = synth.make_scene(n, k, seed=11, knn=knn, noise=1.0, outlier_frac=0.3)
    H = _models(sc, np.random.default_rng(5), extra=3)
    _load(engine, sc)
    if case == "degree_above_register_slots":
        rp, _, _ = engine.get_sym_graph()
        assert np.diff(rp).max() > 48
    engine.set_models(H)
    cost = engine.data_cost()
    lab_ref, e_ref, cyc_ref, _ = oracle.expand(cost, sc.hit_rowptr, sc.hit_col, oracle.potts(LAM))
    try:
        engine.set_tuning(5, grid)
        engine.set_tuning(6, reduce_rounds)
        labels, energy, cycles = engine.expand()
        st = engine.expand_stats()
    finally:
        engine.set_tuning(5, 256)
        engine.set_tuning(6, 2)
    assert energy == e_ref and cycles == cyc_ref and np.array_equal(labels, lab_ref), case
    if case in ("rows_walk_several_sites", "no_reduction_large_core"):
        assert st["core_max"] > grid * 64, "the case did not reach the several-sites-per-row path"
    assert st["moves_run"] < st["moves"], "the converged last cycle should have been skipped on the device"
    assert st["host_syncs"] <= st["cycles"] + 2


def _radius_hits(sc, radius):
    """radiusMatch(1/locality) answered exactly in the reference's float32 (x1,y1,x2,y2) space (M/MultiH.cpp:233-253),
    self hits included like FLANN's (LabelingStep skips them, :537)."""
    pv = np.concatenate([sc.src, sc.dst], axis=1).astype(np.float32)
    diff = pv[:, None, :] - pv[None, :, :]
    sq = diff * diff
    d = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
    hit = d <= np.float32(radius) ** 2
    rowptr = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.int32)
    return rowptr, np.nonzero(hit)[1].astype(np.int32)


@pytest.mark.parametrize("lam,grid", [(0.5, 256), (0.05, 256), (0.05, 2)])
def test_expand_on_a_dense_radius_graph(engine, synth, oracle, lam, grid):
    """The reference's own neighbourhood rule (every correspondence within 1/locality pixels) gives sites HUNDREDS of
    arcs, far above the 48 a solver row keeps in registers, so almost every core site walks its arcs in memory
    (csrc/expand.hip, the `!fast` branches of k_solve).  On that path an arc towards a neighbour decided earlier in the
    move has no capacity in either direction, while that neighbour's flow counter and height word are leftovers of
    older moves: they must never be read as residual capacity (r02 advisor finding).  Several cycles, flow recycling
    on and off, one and several sites per solver row — always the oracle's labels, energy and cycle count."""
    sc = synth.make_scene(1500, 4, seed=31, noise=1.0, outlier_frac=0.3, with_neighbours=False)
    rowptr, col = _radius_hits(sc, 300.0)
    H = _models(sc, np.random.default_rng(31), extra=4)
    engine.set_params(2.6, THR, 0.005, lam, 20)
    try:
        engine.set_correspondences(sc.src, sc.dst, sc.aff)
        engine.set_epipolar(sc.F, sc.e2)
        engine.set_neighbors_csr(rowptr, col)
        rp, _, _ = engine.get_sym_graph()
        assert np.median(np.diff(rp)) > 96, "the scene should put the typical site on the arcs-in-memory path"
        engine.set_models(H)
        cost = engine.data_cost()
        lab_ref, e_ref, cyc_ref, _ = oracle.expand(cost, rowptr, col, oracle.potts(lam))
        assert cyc_ref >= 3
        init = (sc.gt_label + 1).astype(np.int32)
        lab_w_ref, e_w_ref, cyc_w_ref, _ = oracle.expand(cost, rowptr, col, oracle.potts(lam), init_labels=init)
        engine.set_tuning(5, grid)
        for recycle in (1, 0):
            for reduce_rounds in (2, 0):
                engine.set_tuning(11, recycle)
                engine.set_tuning(6, reduce_rounds)
                engine.set_tuning(17, 0 if recycle else 2)          # cascade to its fixed point / capped (the default)
                labels, energy, cycles = engine.expand()
                assert energy == e_ref and cycles == cyc_ref and np.array_equal(labels, lab_ref), (recycle, reduce_rounds)
                labels, energy, cycles = engine.expand(init)
                assert energy == e_w_ref and cycles == cyc_w_ref and np.array_equal(labels, lab_w_ref), (recycle, reduce_rounds, "warm")
        assert engine.expand_stats()["moves_solved"] > 0
    finally:
        engine.set_tuning(5, 256)
        engine.set_tuning(6, 2)
        engine.set_tuning(11, 1)
        engine.set_tuning(17, 2)
        engine.set_params(2.6, THR, 0.005, LAM, 20)


def test_flow_recycling_changes_rounds_not_labels(engine, synth, oracle):
    """From the second cycle on the max-flow of a move starts from the flow the previous expansion on the same label
    ended with (csrc/expand.hip, k_solve).  The read-out of a maximum flow does not depend on where the flow started:
    labels, energy and cycle count are the oracle's with recycling on and off (also with several sites per solver
    row); what recycling changes is the number of relabel rounds."""
    sc = synth.make_scene(8000, 6, seed=21)
    H = sc.H_true * (1.0 + np.random.default_rng(8).normal(0, 1e-4, size=sc.H_true.shape))     # every plane slightly off
    _load(engine, sc)
    engine.set_models(H)
    cost = engine.data_cost()
    lab_ref, e_ref, cyc_ref, _ = oracle.expand(cost, sc.hit_rowptr, sc.hit_col, oracle.potts(LAM))
    assert cyc_ref >= 3, "the scene should need more than one cycle"
    relabels = {}
    try:
        for grid in (256, 4):
            for recycle in (0, 1):
                engine.set_tuning(5, grid)
                engine.set_tuning(11, recycle)
                labels, energy, cycles = engine.expand()
                assert energy == e_ref and cycles == cyc_ref and np.array_equal(labels, lab_ref), (grid, recycle)
                relabels[(grid, recycle)] = engine.expand_stats()["relabels"]
    finally:
        engine.set_tuning(5, 256)
        engine.set_tuning(11, 1)
    assert relabels[(256, 1)] < relabels[(256, 0)], relabels


def test_expand_trace_agrees_with_the_counters(engine, synth):
    """mh_get_expand_trace (diagnostic): one row per move, zero for skipped moves and empty cores; its sums are the
    expansion's counters."""
    sc = synth.make_scene(4000, 4, seed=3)
    _load(engine, sc)
    engine.set_models(_models(sc, np.random.default_rng(3), extra=2))
    engine.data_cost(fetch=False)
    try:
        engine.set_tuning(8, 128)
        engine.expand()
        st = engine.expand_stats()
        tr = engine.expand_trace(128)
    finally:
        engine.set_tuning(8, 0)
    moves = st["moves"]
    assert moves <= 128 and not tr[moves:].any()
    solved = tr[:moves][tr[:moves, 0] > 0]
    assert len(solved) == st["moves_solved"]
    assert solved[:, 0].sum() == st["core_sites"] and solved[:, 0].max() == st["core_max"]
    assert solved[:, 2].sum() == st["relabels"] and solved[:, 5].sum() == st["barriers"]
    assert (solved[:, 7] <= solved[:, 6]).all()                # time inside barriers <= time inside the launch


def test_expand_without_neighbours_is_argmin(engine, synth, oracle):
    sc = synth.make_scene(500, 3, seed=2, with_neighbours=False)
    _load(engine, sc, neighbours=False)
    engine.set_neighbors_csr(np.zeros(sc.n + 1, np.int32), np.zeros(0, np.int32))
    engine.set_models(sc.H_true)
    cost = engine.data_cost()
    labels, energy, _ = engine.expand()
    assert np.array_equal(labels, np.argmin(cost, axis=1))
    assert energy == int(cost.min(axis=1).sum())


def test_sym_graph_matches_oracle(engine, synth, oracle):
    sc = synth.make_scene(1500, 3, seed=6, symmetric=False)
    _load(engine, sc)
    rp, col, w = engine.get_sym_graph()
    rp_r, col_r, w_r = oracle.build_sym_graph(sc.n, sc.hit_rowptr, sc.hit_col)
    assert np.array_equal(rp, rp_r) and np.array_equal(col, col_r) and np.array_equal(w, w_r)
    assert set(np.unique(w)) == {1, 2}       # one-way and mutual kNN hits (SURVEY A-2)


def test_sym_graph_on_the_device_handles_ragged_hit_lists(mh, engine, synth, oracle):
    """The symmetric graph is built on the device (csrc/graph.hip).  Caller-supplied lists with repeated hits, self
    hits, empty rows and a few very long rows (beyond what the per-row LDS sort holds: the host path takes over)
    give exactly the oracle's CSR, multiplicities and — through the expansion — reverse arcs; bad input fails cleanly."""
    rng = np.random.default_rng(11)
    sc = synth.make_scene(2500, 3, seed=12, with_neighbours=False)
    _load(engine, sc, neighbours=False)
    n = sc.n
    for dense_rows in (0, 3):
        rows = []
        for i in range(n):
            d = int(rng.integers(0, 9))
            if i < dense_rows: d = 1500                               # raw row far beyond SYM_MAX_ROW = 1024
            if i % 97 == 5: d = 0
            r = rng.integers(0, n, size=d)
            if d > 2: r[1] = r[0]; r[2] = i                           # a repeated hit and a self hit
            rows.append(r)
        rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        col = np.concatenate(rows).astype(np.int32)
        engine.set_neighbors_csr(rowptr, col)
        rp, cl, w = engine.get_sym_graph()
        rp_o, cl_o, w_o = oracle.build_sym_graph(n, rowptr, col)
        assert np.array_equal(rp, rp_o) and np.array_equal(cl, cl_o) and np.array_equal(w, w_o), dense_rows
        assert w.max() >= 2
        engine.set_models(_models(sc, np.random.default_rng(3), extra=1))
        cost = engine.data_cost()
        labels, energy, cycles = engine.expand()
        lab_ref, e_ref, cyc_ref, _ = oracle.expand(cost, rowptr, col, oracle.potts(LAM))
        assert energy == e_ref and cycles == cyc_ref and np.array_equal(labels, lab_ref), dense_rows
    bad = col.copy(); bad[7] = n
    with pytest.raises(mh.MultiHError) as ei:
        engine.set_neighbors_csr(rowptr, bad)
    assert ei.value.code == -2
    rp_bad = rowptr.copy(); rp_bad[10] = rp_bad[11] + 1
    with pytest.raises(mh.MultiHError) as ei:
        engine.set_neighbors_csr(rp_bad, col)
    assert ei.value.code == -2


@pytest.mark.parametrize("n,k,seed", [(1000, 3, 2), (5000, 3, 1234)])
def test_labeling_step_and_loop(engine, synth, oracle, n, k, seed):
    """LabelingStep (cost -> expand -> shift -> re-estimate), iterated like the reference's
    alternating loop with warm starts: labels and energies bit-exact at every iteration."""
    sc = synth.make_scene(n, k, seed=seed)
    _load(engine, sc)
    H = sc.H_true * (1.0 + np.random.default_rng(seed).normal(0, 1e-4, size=sc.H_true.shape))
    engine.set_models(H)
    lab = np.full(sc.n, -1, dtype=np.int32)
    lab_ref, H_ref = lab.copy(), H.copy()
    for it in range(4):
        warm = it > 0
        lab, energy, cycles = engine.labeling_step(warm, lab)
        lab_ref, H_ref, e_ref, cyc_ref = oracle.labeling_step(sc.src, sc.dst, sc.aff, H_ref, LAM, THR2,
                                                              sc.hit_rowptr, sc.hit_col, warm, sc.F, sc.e2, lab_ref)
        assert energy == e_ref, f"iteration {it}"
        assert np.array_equal(lab, lab_ref), f"iteration {it}"
        Hg = engine.get_models()
        scale = np.max(np.abs(H_ref), axis=1, keepdims=True)
        assert np.max(np.abs(Hg - H_ref) / scale) <= 1e-6
        assert np.array_equal(Hg.view(np.uint64), H_ref.view(np.uint64)), f"iteration {it}"


def test_knn_builder(engine, synth):
    sc = synth.make_scene(2000, 3, seed=12, with_neighbours=False)
    _load(engine, sc, neighbours=False)
    engine.build_neighbors_knn(8)
    rp, col, w = engine.get_sym_graph()
    # brute force in float32 with the kernel's association order and tie rule
    pv = np.concatenate([sc.src, sc.dst], axis=1).astype(np.float32)
    d = np.zeros((sc.n, sc.n), dtype=np.float32)
    diff = pv[:, None, :] - pv[None, :, :]
    sq = diff * diff
    d = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
    np.fill_diagonal(d, np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(sc.n), d.shape), d), axis=1)[:, :8]
    hits = np.zeros((sc.n, sc.n), dtype=np.int32)
    rows = np.repeat(np.arange(sc.n), 8)
    np.add.at(hits, (rows, order.reshape(-1)), 1)
    mult = hits + hits.T
    for i in range(0, sc.n, 97):
        js = col[rp[i]:rp[i + 1]]
        assert np.array_equal(js, np.flatnonzero(mult[i]))
        assert np.array_equal(w[rp[i]:rp[i + 1]], mult[i][js])


@pytest.mark.parametrize("case", ["scene", "duplicates", "line", "clusters", "tiny", "ties", "big"])
def test_knn_through_the_grid_equals_the_exhaustive_pass(engine, synth, case):
    """r05: the k-NN table through a grid over the source image (k_knn_grid: cells walked ring by ring until no unexamined point
    can enter the list; mh_set_tuning key 31) against the exhaustive pass (k_knn) — the symmetric graph built from either is the
    same, entry for entry: ordinary scenes, hundreds of exact duplicates, points on one image row (a grid of zero height),
    a few dense clusters (thousands of points in one cell), fewer points than a wave, integer coordinates (distance ties
    everywhere: the index decides), 50 000 points."""
    rng = np.random.default_rng(abs(hash(case)) % 1000)
    n, k, radius = 3000, 16, 0.0
    if case == "big":
        n = 50000
    sc = synth.make_scene(n, 4, seed=19, with_neighbours=False)
    src, dst = sc.src.copy(), sc.dst.copy()
    if case == "duplicates":
        src[100:700] = src[100]; dst[100:700] = dst[100]
    elif case == "line":
        src[:, 1] = 250.0
    elif case == "clusters":
        c = rng.uniform(100, 900, size=(5, 2))
        src = c[rng.integers(0, 5, n)] + rng.normal(0, 0.05, size=(n, 2)); dst = src + rng.normal(0, 0.05, size=(n, 2))
    elif case == "tiny":
        src, dst, k = src[:20].copy(), dst[:20].copy(), 8
    elif case == "ties":
        src = np.floor(src / 25.0) * 25.0; dst = np.floor(dst / 25.0) * 25.0; radius = 60.0
    engine.set_correspondences(src, dst)
    got = {}
    try:
        for grid in (1, 0):
            engine.set_tuning(31, grid)
            if radius > 0:
                engine.build_neighbors_knn(k, radius=radius)
            else:
                engine.build_neighbors_knn(k)
            got[grid] = engine.get_sym_graph()
    finally:
        engine.set_tuning(31, 1)
    for a, b in zip(got[1], got[0]):
        assert np.array_equal(a, b), case
    assert got[1][0][-1] >= src.shape[0] * min(k, 4) or case == "ties"


def test_knn_within_the_reference_radius(engine, synth):
    """mh_build_neighbors_knn_radius (the host class's default neighbourhood): the k nearest hits, of which only those
    within the radius survive — checked against a float32 brute force with the kernel's association order."""
    sc = synth.make_scene(1500, 3, seed=13, with_neighbours=False)
    _load(engine, sc, neighbours=False)
    k, r = 12, 45.0
    engine.build_neighbors_knn(k, radius=r)
    rp, col, w = engine.get_sym_graph()
    pv = np.concatenate([sc.src, sc.dst], axis=1).astype(np.float32)
    diff = pv[:, None, :] - pv[None, :, :]
    sq = diff * diff
    d = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
    np.fill_diagonal(d, np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(sc.n), d.shape), d), axis=1)[:, :k]
    hits = np.zeros((sc.n, sc.n), dtype=np.int32)
    r2 = np.float32(r) * np.float32(r)
    for i in range(sc.n):
        js = order[i][d[i, order[i]] <= r2]
        hits[i, js] += 1
    assert 0 < hits.sum() < sc.n * k, "the radius must cut some of the k nearest hits for this test to mean anything"
    mult = hits + hits.T
    for i in range(0, sc.n, 53):
        js = col[rp[i]:rp[i + 1]]
        assert np.array_equal(js, np.flatnonzero(mult[i]))
        assert np.array_equal(w[rp[i]:rp[i + 1]], mult[i][js])
    engine.build_neighbors_knn(k)                                  # no cut: every query keeps its k hits
    rp2, _, w2 = engine.get_sym_graph()
    assert w2.sum() == 2 * sc.n * k


def test_radius_neighbourhood_is_the_exact_reference_rule(mh, engine, synth, oracle):
    """mh_build_neighbors_radius: the hit list radiusMatch(1/locality) asks for (M/MultiH.cpp:252-253),
    exact: float32 squared distance <= r^2, self included; fed through the same setNeighbors
    multiplicity rule as a caller-supplied list (oracle build_sym_graph).  The bound on the hit count
    fails cleanly and leaves the previous graph in place."""
    sc = synth.make_scene(1800, 3, seed=8, with_neighbours=False)
    _load(engine, sc, neighbours=False)
    r = 60.0
    pv = np.concatenate([sc.src, sc.dst], axis=1).astype(np.float32)
    diff = pv[:, None, :] - pv[None, :, :]
    sq = diff * diff
    d = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
    hit = d <= np.float32(r) * np.float32(r)
    assert hit.diagonal().all()
    rowptr = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.int32)
    col = np.nonzero(hit)[1].astype(np.int32)
    hits = engine.build_neighbors_radius(r)
    assert hits == col.size
    rp, cl, w = engine.get_sym_graph()
    rp_o, cl_o, w_o = oracle.build_sym_graph(sc.n, rowptr, col)
    assert np.array_equal(rp, rp_o) and np.array_equal(cl, cl_o) and np.array_equal(w, w_o)
    assert (w == 2).all()                       # a radius rule is symmetric: every pair is found from both sides
    with pytest.raises(mh.MultiHError) as ei:
        engine.build_neighbors_radius(r, max_hits=col.size - 1)
    assert ei.value.code == -5
    rp2, cl2, _ = engine.get_sym_graph()
    assert np.array_equal(rp2, rp) and np.array_equal(cl2, cl)
    # and the labeling on that graph equals the oracle's on the same hit list
    engine.set_models(_models(sc, np.random.default_rng(3), extra=2))
    cost = engine.data_cost()
    labels, energy, cycles = engine.expand()
    lab_ref, e_ref, cyc_ref, _ = oracle.expand(cost, rowptr, col, oracle.potts(LAM))
    assert energy == e_ref and cycles == cyc_ref and np.array_equal(labels, lab_ref)


def test_fp64_division_and_sqrt_are_ieee(engine, synth, oracle):
    """The bit-exactness argument rests on the device's FP64 divide being correctly rounded.
    Stress it through the residual kernel with adversarial magnitudes."""
    rng = np.random.default_rng(99)
    n = 4096
    src = rng.uniform(-1e3, 1e3, size=(n, 2)) * 10.0 ** rng.integers(-3, 4, size=(n, 1))
    dst = rng.uniform(-1e3, 1e3, size=(n, 2))
    H = rng.normal(size=(64, 9)) * 10.0 ** rng.integers(-6, 7, size=(64, 9))
    engine.set_correspondences(src, dst)
    engine.set_models(H)
    with np.errstate(all="ignore"):
        R, _ = engine.residual_matrix(THR2, fetch_counts=False)
        R_ref = oracle.residual_matrix(src, dst, H)
    nan = np.isnan(R_ref)
    assert np.array_equal(np.isnan(R), nan)
    assert np.array_equal(R[~nan].view(np.uint64), R_ref[~nan].view(np.uint64))


@pytest.mark.parametrize("symmetric", [False, True])
def test_shared_reciprocal_precondition_boundaries(engine, oracle, symmetric):
    """The residual sweep replaces the two IEEE divisions by one shared reciprocal when per-model,
    per-point and per-pair preconditions hold (csrc/mh_device.hpp) and falls back to the full
    division otherwise.  Sit exactly on those boundaries — coefficients and coordinates around
    2^120, targets around 2^-450, denominators around 2^-255 — and demand the oracle's bits on
    both sides of each of them."""
    rng = np.random.default_rng(4242)
    n, m = 2048, 192
    pe = np.array([-460, -451, -450, -449, -300, -20, 0, 0, 0, 7, 10, 118, 119, 120, 121, 300])
    src = rng.uniform(1.0, 2.0, size=(n, 2)) * np.exp2(rng.choice(pe, size=(n, 2)).astype(np.float64))
    dst = rng.uniform(1.0, 2.0, size=(n, 2)) * np.exp2(rng.choice(pe, size=(n, 2)).astype(np.float64))
    src *= rng.choice([-1.0, 1.0], size=src.shape)
    dst *= rng.choice([-1.0, 1.0], size=dst.shape)
    src[:64] = rng.uniform(0, 1000, size=(64, 2)); dst[:64] = rng.uniform(0, 1000, size=(64, 2))   # ordinary pixels
    src[64:72] = 0.0; dst[72:80] = 0.0
    he = np.array([-300, -256, -255, -254, -60, -3, 0, 0, 0, 5, 60, 119, 120, 121, 256, 257, 258])
    H = rng.normal(size=(m, 9)) * np.exp2(rng.choice(he, size=(m, 9)).astype(np.float64))
    # denominators straddling 2^-255: s = h8 exactly (h6 = h7 = 0), |h8| = 2^-255 * {1-eps, 1, 1+eps}
    for i, f in enumerate((1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, -1.0, 2.0 ** -1, 2.0)):
        H[i] = [1e-250, 0, 3e-252, 0, 1e-250, -2e-251, 0, 0, f * 2.0 ** -255]
    H[8] = [1, 0, 0, 0, 1, 0, 0, 0, np.inf]
    H[9] = [1, 0, 0, 0, np.nan, 0, 0, 0, 1]
    engine.set_correspondences(src, dst)
    engine.set_models(H)
    engine.set_residual_mode(symmetric)
    try:
        with np.errstate(all="ignore"):
            R, cnt = engine.residual_matrix(THR2)
            R_ref = (oracle.residual_matrix_sym if symmetric else oracle.residual_matrix)(src, dst, H)
            cnt2 = engine.score(THR2)
    finally:
        engine.set_residual_mode(False)
    nan = np.isnan(R_ref)
    assert np.array_equal(np.isnan(R), nan)
    assert np.array_equal(R[~nan].view(np.uint64), R_ref[~nan].view(np.uint64))
    with np.errstate(all="ignore"):
        ref_cnt = (R_ref < THR2).sum(axis=1)
    assert np.array_equal(cnt, ref_cnt) and np.array_equal(cnt2, ref_cnt)
    assert 0.05 < np.isfinite(R_ref).mean() < 0.9999 and ref_cnt.sum() > 0     # both regimes present


_FORMS = ("sweep", "sweep_sym", "score", "score_masked", "score_sym", "score_sym_masked")
_form_inputs = {}


def _form_edge_inputs(synth, n):
    """65 models on n points, off the lean path in every way it can be left: a source coordinate outside the fast
    division's precondition (its wave tile takes the checked sweep), a model whose horizon runs through the data (not
    `far`) and a model that fails model_pre (the fallback division).  Made once per n, never modified."""
    if n not in _form_inputs:
        sc = synth.make_scene(n, 3, seed=n, with_neighbours=False)
        rng = np.random.default_rng(n)
        src, dst = sc.src.copy(), sc.dst.copy()
        src[17, 0] = 1e100
        H = _models(sc, rng, extra=62)
        H[3] = [1, 0, 0, 0, 1, 0, 1e-3, -1e-3, 0]
        H[5] = [1e150, 0, 0, 0, 1e150, 0, 0, 0, 1e150]
        mask = (rng.random(n) < 0.6).astype(np.uint8)
        mask[-1] = 1                                    # the odd tail point counts
        assert H.shape[0] == 65
        for a in (src, dst, H, mask):
            a.setflags(write=False)
        _form_inputs[n] = (src, dst, H, mask)
    return _form_inputs[n]


@pytest.mark.parametrize("n", [1023, 2049])
@pytest.mark.parametrize("form", _FORMS)
def test_every_product_form_of_the_sweep_at_partial_shapes(engine, synth, oracle, form, n):
    """The six product configurations of the residual sweep (residual.hip, namespace cfg: Sweep, SweepSym, Score,
    ScoreMasked, ScoreSym, ScoreSymMasked), each against the oracle, bit for bit, where every loop has a partial last
    trip: n = 1023 is an odd tail inside the last 16-byte chunk of ONE partial 1 024-point tile (one point slice: counts are
    written directly), n = 2049 three tiles, the last holding one point (three slices: counts through the atomic path);
    65 models leave a one-model block behind 64 (Sweep) and behind 4 x 16 (the others)."""
    src, dst, H, mask = _form_edge_inputs(synth, n)
    sym = "sym" in form
    m = mask if form.endswith("masked") else None
    engine.set_correspondences(src, dst)
    engine.set_models(H)
    engine.set_residual_mode(sym)
    engine.set_tuning(15, 0)                # the forward score through the FP64 sweep, not the FP32 pre-test
    try:
        with np.errstate(all="ignore"):
            if form.startswith("sweep"):
                R, cnt = engine.residual_matrix(THR2)
                R_ref = (oracle.residual_matrix_sym if sym else oracle.residual_matrix)(src, dst, H)
                assert R.shape == R_ref.shape == (65, n)
                assert np.array_equal(R.view(np.uint64), R_ref.view(np.uint64))
            else:
                cnt = engine.score(THR2, mask=m)
            cnt_ref = (oracle.score_sym if sym else oracle.score)(src, dst, H, THR2, mask=m)
    finally:
        engine.set_tuning(15, 1)
        engine.set_residual_mode(False)
    assert np.array_equal(cnt, cnt_ref)
    assert cnt_ref.max() > n // 8 and cnt_ref[5] < n


def test_product_library_carries_no_measurement_variants(mh, engine, synth, oracle):
    """The residual / score kernel variants used for the A/B evidence of HISTORY.md section 7 — one of them, fused
    multiply-adds, is not bit-exact — live only in the measurement library (build.py --tuning).  The product library
    refuses to select them, so nothing reachable through its ABI can change a result; a sweep over points whose
    bounding box lets the per-model |s| proof succeed AND points that defeat it stays bit-exact."""
    sc = synth.make_scene(3000, 3, seed=31, with_neighbours=False)
    H = _models(sc, np.random.default_rng(31), extra=20)
    _load(engine, sc, neighbours=False)
    engine.set_models(H)
    for key in (0, 1):
        for value in (1, 3, 10, 104):
            with pytest.raises(mh.MultiHError) as ei:
                engine.set_tuning(key, value)
            assert ei.value.code == -2                     # MH_ERR_INVALID
        engine.set_tuning(key, 0)
    R, cnt = engine.residual_matrix(THR2)
    R_ref = oracle.residual_matrix(sc.src, sc.dst, H)
    assert np.array_equal(R.view(np.uint64), R_ref.view(np.uint64))
    # models whose horizon (s = 0) crosses the data: the bounding-box proof fails for them and the per-pair check runs
    Hh = H.copy()
    Hh[::2, 6] = -1.0 / 500.0
    Hh[::2, 7] = 0.0
    Hh[::2, 8] = 1.0                                      # s = 1 - x / 500 changes sign inside the 1000-px image
    engine.set_models(Hh)
    with np.errstate(all="ignore"):
        R2, cnt2 = engine.residual_matrix(THR2)
        R2_ref = oracle.residual_matrix(sc.src, sc.dst, Hh)
    nan = np.isnan(R2_ref)
    assert np.array_equal(np.isnan(R2), nan) and np.array_equal(R2[~nan].view(np.uint64), R2_ref[~nan].view(np.uint64))
    assert np.array_equal(cnt2, engine.score(THR2))


# ---- committed golden fixtures (labels pinned by the reference's own GCO build) -------------
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("tag", ["n64_k2", "n1000_k3", "n5000_k3"])
def test_engine_matches_golden_labeling(engine, tag):
    g = np.load(os.path.join(GOLDEN, f"labeling_{tag}.npz"))
    engine.set_correspondences(g["src"], g["dst"], g["aff"])
    engine.set_epipolar(g["F"], g["e2"])
    engine.set_neighbors_csr(g["hit_rowptr"], g["hit_col"])
    engine.set_models(g["H"])
    assert np.array_equal(engine.data_cost(), g["cost"])
    R, cnt = engine.residual_matrix(float(g["thr"]) ** 2)
    assert np.array_equal(R[:, :64].view(np.uint64), g["residual_first64"].view(np.uint64))
    assert np.array_equal(cnt, g["counts"])
    labels, energy, cycles = engine.expand()
    assert energy == int(g["energy_ref"]) and np.array_equal(labels, g["labels_ref"])
    assert cycles == int(g["cycles"])
    labels_w, energy_w, _ = engine.expand(g["init_warm"])
    assert energy_w == int(g["energy_warm"]) and np.array_equal(labels_w, g["labels_warm"])
    H_re = engine.reestimate(g["labels_ref"] - 1)
    scale = np.max(np.abs(g["H_reestimated"]), axis=1, keepdims=True)
    assert np.max(np.abs(H_re - g["H_reestimated"]) / scale) <= 1e-6


def test_engine_matches_golden_dlt(engine):
    g = np.load(os.path.join(GOLDEN, "dlt_n500_m256.npz"))
    engine.set_correspondences(g["src"], g["dst"])
    engine.propose_dlt4(int(g["seed"]), int(g["first"]), g["idx"].shape[0])
    assert np.array_equal(engine.get_samples(), g["idx"])
    good = g["witness"] > 1e-6
    assert np.max(np.abs(engine.get_models()[good] - g["H"][good])) <= 1e-6


# ---- BASELINE full size: size-independent properties ----------------------------------------
def test_full_size_properties_50k_x_100k(engine, synth, oracle):
    """BASELINE configs[2] (50 000 correspondences, 100 000 hypotheses): the 40 GB matrix cannot be
    compared entry by entry on the host, so check (a) sampled row blocks bit-exactly against the
    oracle, (b) fused counts == counts of the store-free score kernel == oracle on sampled rows,
    (c) scale invariance: multiplying every model by a power of two leaves R bit-identical,
    (d) every count is within [0, N] and the best hypotheses have plausible support."""
    N, M = 50000, 100000
    sc = synth.make_scene(N, 10, seed=1234, with_neighbours=False)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.propose_dlt4(1234, 0, M)
    H = engine.get_models()
    _, cnt = engine.residual_matrix(THR2, fetch_R=False)
    assert np.array_equal(engine.score(THR2), cnt)
    assert cnt.min() >= 0 and cnt.max() <= N and cnt.max() > 1000
    blocks = [(0, 24), (M // 2 - 7, 24), (M - 24, 24)]
    kept = {}
    with np.errstate(all="ignore"):
        for first, count in blocks:
            rows = engine.get_residual_rows(first, count)
            ref = oracle.residual_matrix(sc.src, sc.dst, H[first:first + count])
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(rows), nan)
            assert np.array_equal(rows[~nan].view(np.uint64), ref[~nan].view(np.uint64))
            assert np.array_equal(cnt[first:first + count], oracle.score(sc.src, sc.dst, H[first:first + count], THR2))
            kept[first] = rows
    engine.set_models(H * 0.125)
    _, cnt2 = engine.residual_matrix(THR2, fetch_R=False)
    assert np.array_equal(cnt2, cnt)
    for first, count in blocks:
        rows = engine.get_residual_rows(first, count)
        a, b = rows, kept[first]
        both = ~(np.isnan(a) & np.isnan(b))
        assert np.array_equal(a[both].view(np.uint64), b[both].view(np.uint64))


def test_full_size_every_stored_entry_is_recounted_on_the_device():
    """The whole 40 GB matrix, not samples of it: torch (plumbing — a zero-copy view of the engine's buffer) counts, row by
    row, the stored entries below thr^2 and the entries that are not NaN; the first must equal the kernel's fused counts for
    all 100 000 rows — a row segment that was never stored, or stored in the wrong row, cannot hide behind the sampled
    blocks of the test above (r05: the work item went from 16 to 64 models) — and with the matrix pre-filled with NaN the
    second shows every entry written.  A process of its own (tests/full_matrix_recount_worker.py): torch has to initialise
    its HIP runtime before the engine's library is loaded."""
    import subprocess, sys
    pytest.importorskip("torch")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "full_matrix_recount_worker.py")
    r = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "RECOUNT OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_full_size_symmetric_transfer_50k_x_100k(engine, synth, oracle):
    """r05: the symmetric transfer error at BASELINE configs[2] size (the 40 GB matrix in MH_RESIDUAL_SYMMETRIC mode): sampled
    row blocks bit-exactly against the oracle's restatement, fused counts == store-free score == oracle on those rows, every
    entry >= the forward residual of the same pair (a sum of two squares against one of them), counts <= the forward counts."""
    N, M = 50000, 100000
    sc = synth.make_scene(N, 10, seed=1234, with_neighbours=False)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.propose_dlt4(1234, 0, M)
    H = engine.get_models()
    _, cnt_fwd = engine.residual_matrix(THR2, fetch_R=False)
    blocks = [(0, 16), (M // 2 - 5, 16), (M - 16, 16)]
    fwd = {first: engine.get_residual_rows(first, count) for first, count in blocks}
    engine.set_residual_mode(True)
    try:
        _, cnt = engine.residual_matrix(THR2, fetch_R=False)
        assert np.array_equal(engine.score(THR2), cnt)
        assert (cnt <= cnt_fwd).all() and cnt.max() > 1000
        with np.errstate(all="ignore"):
            for first, count in blocks:
                rows = engine.get_residual_rows(first, count)
                ref = oracle.residual_matrix_sym(sc.src, sc.dst, H[first:first + count])
                nan = np.isnan(ref)
                assert np.array_equal(np.isnan(rows), nan)
                assert np.array_equal(rows[~nan].view(np.uint64), ref[~nan].view(np.uint64))
                assert np.array_equal(cnt[first:first + count], oracle.score_sym(sc.src, sc.dst, H[first:first + count], THR2))
                ok = ~nan & ~np.isnan(fwd[first])
                assert (rows[ok] >= fwd[first][ok]).all()
    finally:
        engine.set_residual_mode(False)


def test_full_size_labeling_equals_the_reference_gco(engine, synth, oracle):
    """BASELINE's 50 000 correspondences / 10 planes: one LabelingStep on the GPU (data cost, alpha-
    expansion with 0.9 M neighbour hits, label shift) against the reference's own GCoptimization
    sources compiled unmodified (oracle/_ref) with its callback data cost — labels and energy
    identical."""
    if oracle.ref() is None:
        pytest.skip("oracle/_ref is not built (needs /root/reference at build time)")
    sc = synth.make_scene(50000, 10, seed=1234)
    _load(engine, sc)
    H = sc.H_true * (1.0 + np.random.default_rng(0).normal(0, 1e-4, size=sc.H_true.shape))
    engine.set_models(H)
    lab, energy, cycles = engine.labeling_step(False, np.full(sc.n, -1, np.int32))
    lab_r, e_r = oracle.ref_expand_formula(sc.src, sc.dst, H, LAM, THR2, sc.hit_rowptr, sc.hit_col)
    assert int(energy) == e_r and np.array_equal(lab_r - 1, lab)
    assert cycles >= 2 and (lab >= 0).sum() > 30000
    # the same step with every solver row owning several sites (48 workgroups for cores of ten thousand sites) and
    # with the flows recycled or not: the schedule never shows in the result
    try:
        for grid, recycle in ((48, 1), (48, 0), (256, 0)):
            engine.set_tuning(5, grid)
            engine.set_tuning(11, recycle)
            engine.set_models(H)
            lab2, energy2, cycles2 = engine.labeling_step(False, np.full(sc.n, -1, np.int32))
            assert int(energy2) == e_r and cycles2 == cycles and np.array_equal(lab2, lab), (grid, recycle)
            if grid == 48:
                assert engine.expand_stats()["core_max"] > 48 * 64
    finally:
        engine.set_tuning(5, 256)
        engine.set_tuning(11, 1)


@pytest.mark.parametrize("n,planes,M,max_models", [(3000, 3, 4000, 12), (5000, 3, 10000, 16)])
def test_greedy_selection_on_the_device(engine, synth, oracle, n, planes, M, max_models):
    """mh_select_greedy (csrc/select.hip) against the selection spelt out on the host with the primitives it replaced —
    masked re-score of the WHOLE batch, first maximum, the winner's inliers leave the mask: same hypotheses in the same
    order with the same counts, same homographies, same final mask.  (The device version prunes hypotheses that
    dropped below `need`; counts only fall, so that can never change a pick.)  And the loop issues no host<->device
    copy: the count of explicit copies does not depend on the number of rounds."""
    sc = synth.make_scene(n, planes, seed=31, with_neighbours=False)
    _load(engine, sc, neighbours=False)
    need = 20
    engine.propose_dlt4(77, 0, M)
    H_all = engine.get_models()
    mask = np.ones(n, dtype=np.uint8)
    picks, counts_ref = [], []
    for _ in range(max_models):
        c = engine.score(THR2, mask)
        best = int(np.argmax(c))
        if c[best] < need:
            break
        picks.append(best)
        counts_ref.append(int(c[best]))
        lab = engine.inliers_of_model(best, THR2, 0, np.full(n, -1, np.int32))
        mask[(lab == 0)] = 0
    assert len(picks) >= planes
    engine.copy_stats(reset=True)
    H, counters, counts, mask_out = engine.select_greedy(THR2, need, max_models, np.ones(n, dtype=np.uint8))
    copies_full = engine.copy_stats(reset=True)
    assert counters.tolist() == picks and counts.tolist() == counts_ref
    assert np.array_equal(H.view(np.uint64), H_all[picks].view(np.uint64))
    assert np.array_equal(mask_out, mask)
    # ... and against the ORACLE's own sequential selection (oracle/mh_oracle.cpp section 12) over the oracle's own DLT
    # of the same counter-RNG tuples: same hypotheses in the same order, same counts, same final support set
    H_o_all, _, _ = oracle.dlt4(sc.src, sc.dst, oracle.sample4(77, 0, M, n))
    Hs_o, idx_o, cnt_o, mask_o = oracle.select_greedy(sc.src, sc.dst, H_o_all, THR2, need, max_models)
    assert idx_o.tolist() == picks and cnt_o.tolist() == counts_ref and np.array_equal(mask_o, mask_out)
    assert np.max(np.abs(H - Hs_o)) <= 1e-6
    # fewer rounds, same number of copies (mask up; H, counters, mask and one check word down)
    engine.select_greedy(THR2, need, 2, np.ones(n, dtype=np.uint8))
    copies_two = engine.copy_stats(reset=True)
    assert copies_full == copies_two and sum(copies_full) <= 5
    # a restricted support mask in: only those points are ever counted or claimed
    half = (np.arange(n) % 2).astype(np.uint8)
    H2, counters2, counts2, m2 = engine.select_greedy(THR2, need, max_models, half)
    assert np.all(m2[half == 0] == 0) and counts2[0] == engine.score(THR2, half)[counters2[0]]


# ---- host class MultiH over the C ABI (integration) -----------------------------------------
def test_host_multih_process_loop(mh, engine_lib, synth):
    import ctypes as C
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    sc = synth.make_scene(5000, 3, seed=1234)                        # BASELINE configs[1] scale
    n = sc.n
    dp = C.POINTER(C.c_double)
    labels = np.full(n, -7, dtype=np.int32)
    Hout = np.zeros((64, 9))
    it, en, secs = C.c_int(0), C.c_double(0), C.c_double(0)
    src, dst, aff = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff))
    F, e2 = np.ascontiguousarray(sc.F), np.ascontiguousarray(sc.e2)
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), n,
                             F.ctypes.data_as(dp), e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.2),
                             C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(1234), 10000, 16, 0,
                             None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)), Hout.ctypes.data_as(dp), 64,
                             C.byref(it), C.byref(en), C.byref(secs), 0, 4)
    assert k >= 3, "the three planes must be found"
    assert labels.min() >= -1 and labels.max() < k
    assert 1 <= it.value <= 500
    # each ground-truth plane is dominated by one label, and different planes by different labels
    dom = []
    for p in range(3):
        lab_p = labels[sc.gt_label == p]
        vals, counts = np.unique(lab_p[lab_p >= 0], return_counts=True)
        assert counts.max() > 0.5 * (sc.gt_label == p).sum()
        dom.append(int(vals[np.argmax(counts)]))
    assert len(set(dom)) == 3
    # fewer than 8 points: the reference's error path (Process returns false)
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), 7,
                             F.ctypes.data_as(dp), e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.2),
                             C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(1), 100, 4, 0, None, 0,
                             labels.ctypes.data_as(C.POINTER(C.c_int)), Hout.ctypes.data_as(dp), 64, None, None, None, 0, 4)
    assert k == -1


def test_degenerate_tail_labels_the_original_points(mh, engine_lib, synth, oracle):
    """HandleDegenerateCase reached from the END of Process() (at most one cluster left, M/MultiH.cpp:88-94) after the
    engine's own front half has FILTERED the points: the reference fits and labels the ORIGINAL correspondences
    (:719-741), so labels.size() is the original count and label i belongs to original point i.  (Round-1 bug: the
    engine still held the filtered set, the labels were written in filtered order.)  One plane plus gross outliers,
    no SetEpipolarGeometry; the outliers make the affine-consistency filter drop points."""
    import ctypes as C
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    sc = synth.make_scene(3000, 1, seed=5, outlier_frac=0.35)
    n = sc.n
    dp = C.POINTER(C.c_double)
    labels = np.full(n, -7, dtype=np.int32)
    Hout = np.zeros((8, 9))
    src, dst, aff = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff))
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), n,
                             None, None, C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5), 20,
                             C.c_ulonglong(99), 4000, 8, 0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 8, None, None, None, 0, 4)
    assert k == 1, "a single plane: the loop ends with one cluster and Process() takes the degenerate tail"
    assert set(np.unique(labels)) <= {-1, 0}, "every ORIGINAL point carries a label (none left at the -7 fill)"
    # label 0 <=> forward-transfer inlier of the returned homography, evaluated on the ORIGINAL point of that index
    with np.errstate(all="ignore"):
        d2 = oracle.residual_matrix(sc.src, sc.dst, Hout[:1])[0]
    assert np.array_equal(labels == 0, d2 < THR2)
    assert (labels == 0).sum() > 0.5 * (sc.gt_label == 0).sum()


def test_barrsmith_real_data_end_to_end(mh, engine_lib):
    """BASELINE configs[0] data (the reference's only bundled correspondence set) through the host
    class on the GPU.  F / e2 come from a numpy 8-point RANSAC (tests/epipolar_np.py) standing in
    for the OpenCV front half.  The reference's own run is not bit-reproducible (OpenCV RANSAC,
    FLANN, MSVC rand()), so this is a plausibility check against its checked-in result file: the
    same number of planes, and its dominant plane is recovered as one label."""
    import ctypes as C
    import epipolar_np as E
    g = np.load(os.path.join(GOLDEN, "barrsmith.npz"))
    pts, res = g["points"], g["result"]
    F, inl = E.fundamental_ransac(pts[:, 0:2], pts[:, 2:4], thr=2.0, iters=3000, seed=1)
    assert inl.sum() > 1000
    src, dst, aff = (np.ascontiguousarray(pts[inl][:, a:b]) for a, b in ((0, 2), (2, 4), (4, 8)))
    Fc, e2 = np.ascontiguousarray(F.reshape(9)), np.ascontiguousarray(E.epipole2(F))
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    n = len(src)
    dp = C.POINTER(C.c_double)
    labels = np.full(n, -7, dtype=np.int32)
    Hout = np.zeros((64, 9))
    it = C.c_int(0)
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), n,
                             Fc.ctypes.data_as(dp), e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.2),
                             C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(1234), 20000, 16, 0, None, 0,
                             labels.ctypes.data_as(C.POINTER(C.c_int)), Hout.ctypes.data_as(dp), 64,
                             C.byref(it), None, None, 0, 4)
    assert 3 <= k <= 8                                   # the reference's result has 5 planes
    assert labels.min() >= -1 and labels.max() < k
    key = {(round(a, 3), round(b, 3)): i for i, (a, b) in enumerate(src)}
    rows = np.array([key.get((round(a, 3), round(b, 3)), -1) for a, b in res[:, :2]])
    ok = rows >= 0
    assert ok.mean() > 0.9
    ref_lab, ours = res[ok, 8].astype(int), labels[rows[ok]]
    dom = ours[ref_lab == 1]                             # the reference's largest plane (514 points)
    vals, cnts = np.unique(dom[dom >= 0], return_counts=True)
    assert cnts.max() > 0.8 * dom.size


def test_harness_file_formats(mh, synth, tmp_path):
    """multih_harness: the reference's cached-correspondence format in (8 numbers per line,
    M/main.cpp:380-396) and its result format out (9 numbers per line, :429-446)."""
    import subprocess
    sc = synth.make_scene(1500, 3, seed=21, with_neighbours=False)
    inp, out, epi = tmp_path / "corr.txt", tmp_path / "result.txt", tmp_path / "epi.txt"
    np.savetxt(inp, np.concatenate([sc.src, sc.dst, sc.aff], axis=1), fmt="%.10g")
    np.savetxt(epi, np.concatenate([sc.F, sc.e2])[None, :], fmt="%.17g")
    exe = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    r = subprocess.run([exe, str(inp), str(out), "--epipolar", str(epi), "--hypotheses", "5000"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "[Multi-H] Processing has been started." in r.stdout
    res = np.loadtxt(out)
    assert res.shape == (1500, 9)
    assert np.allclose(res[:, :2], sc.src, rtol=1e-5)
    labels = res[:, 8].astype(int)
    assert labels.min() >= -1 and labels.max() >= 2
    # the reference's radius neighbourhood (1/locality = 40 px here) instead of k-NN
    out2 = tmp_path / "result_radius.txt"
    r = subprocess.run([exe, str(inp), str(out2), "--epipolar", str(epi), "--hypotheses", "5000",
                        "--locality", "0.025", "--neighbourhood", "radius"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res2 = np.loadtxt(out2)
    assert res2.shape == (1500, 9) and res2[:, 8].max() >= 2
    # too few correspondences: the reference's error path
    np.savetxt(inp, np.concatenate([sc.src, sc.dst, sc.aff], axis=1)[:5], fmt="%.10g")
    r = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Features are not set" in r.stderr


# ---- error behaviour and edge cases of the C ABI ---------------------------------------------
def test_capi_error_paths(mh, engine, synth):
    sc = synth.make_scene(100, 2, seed=1)
    with pytest.raises(mh.MultiHError) as ei:              # nothing set yet
        engine.score(THR2)
    assert ei.value.code == -4
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    with pytest.raises(mh.MultiHError) as ei:              # no models yet
        engine.data_cost()
    assert ei.value.code == -4
    engine.set_models(sc.H_true)
    with pytest.raises(mh.MultiHError) as ei:              # expansion without a neighbour graph
        engine.data_cost(); engine.expand()
    assert ei.value.code == -4
    with pytest.raises(mh.MultiHError) as ei:              # re-estimation without F
        engine.reestimate(np.zeros(sc.n, np.int32))
    assert ei.value.code == -4
    engine.set_epipolar(sc.F, sc.e2)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    with pytest.raises(mh.MultiHError) as ei:              # label outside 0..Nh
        engine.data_cost(); engine.expand(np.full(sc.n, 7, np.int32))
    assert ei.value.code == -2
    with pytest.raises(mh.MultiHError) as ei:              # neighbour index out of range
        engine.set_neighbors_csr(sc.hit_rowptr, np.full_like(sc.hit_col, sc.n + 5))
    assert ei.value.code == -2
    with pytest.raises(mh.MultiHError):
        engine.inliers_of_model(99, THR2, 0, np.zeros(sc.n, np.int32))
    with pytest.raises(mh.MultiHError):
        engine.build_neighbors_knn(64)
    with pytest.raises(mh.MultiHError) as ei:              # stale cost after the model set changed
        engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col); engine.data_cost(); engine.set_models(sc.H_true[:1]); engine.expand()
    assert ei.value.code == -4
    with pytest.raises(mh.MultiHError):
        mh.Engine(device=99)


def test_tiny_and_ragged_inputs(engine, synth, oracle):
    # 4 correspondences are enough to propose; one model; counts of an empty mask
    sc = synth.make_scene(4, 1, seed=3, outlier_frac=0.0, with_neighbours=False)
    engine.set_correspondences(sc.src, sc.dst)
    engine.propose_dlt4(5, 0, 3)
    assert np.array_equal(engine.get_samples(), oracle.sample4(5, 0, 3, 4))
    assert sorted(engine.get_samples()[0].tolist()) == [0, 1, 2, 3]
    R, cnt = engine.residual_matrix(THR2)
    assert R.shape == (3, 4)
    # sizes around the tile boundaries of the sweep (256*PPL points, 16 models)
    for n, m in ((1023, 15), (1024, 16), (1025, 17), (2049, 33)):
        sc = synth.make_scene(n, 2, seed=n, with_neighbours=False)
        H = np.random.default_rng(n).normal(size=(m, 9)) * 0.01 + np.eye(3).reshape(9)
        engine.set_correspondences(sc.src, sc.dst)
        engine.set_models(H)
        with np.errstate(all="ignore"):
            R, cnt = engine.residual_matrix(THR2)
            Rr = oracle.residual_matrix(sc.src, sc.dst, H)
        nan = np.isnan(Rr)
        assert np.array_equal(R[~nan].view(np.uint64), Rr[~nan].view(np.uint64))
        assert np.array_equal(cnt, oracle.score(sc.src, sc.dst, H, THR2))
        assert np.array_equal(engine.score(THR2), cnt)


def test_two_engines_and_reuse(mh, engine_lib, synth, oracle):
    """Two engines on the same device do not share state; an engine can be re-targeted to a new
    correspondence set (buffers grow/shrink correctly)."""
    a = mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20)
    b = mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20)
    try:
        s1 = synth.make_scene(700, 2, seed=1, with_neighbours=False)
        s2 = synth.make_scene(3000, 3, seed=2, with_neighbours=False)
        a.set_correspondences(s1.src, s1.dst); b.set_correspondences(s2.src, s2.dst)
        a.set_models(s1.H_true); b.set_models(s2.H_true)
        ca, cb = a.score(THR2), b.score(THR2)
        assert np.array_equal(ca, oracle.score(s1.src, s1.dst, s1.H_true, THR2))
        assert np.array_equal(cb, oracle.score(s2.src, s2.dst, s2.H_true, THR2))
        a.set_correspondences(s2.src, s2.dst); a.set_models(s2.H_true)          # grow
        assert np.array_equal(a.score(THR2), cb)
        b.set_correspondences(s1.src, s1.dst); b.set_models(s1.H_true)          # shrink
        assert np.array_equal(b.score(THR2), ca)
    finally:
        a.close(); b.close()


def test_symmetric_transfer_mode(engine, synth, oracle):
    """north_star's symmetric-transfer residual (extension, no reference counterpart): bit-exact
    against the oracle's definition; the default (forward, reference formula) is restored after."""
    sc = synth.make_scene(3001, 3, seed=17, with_neighbours=False)
    H = _models(sc, np.random.default_rng(2), extra=14)
    _load(engine, sc, neighbours=False)
    engine.set_models(H)
    R_fwd, c_fwd = engine.residual_matrix(THR2)
    engine.set_residual_mode(True)
    R, cnt = engine.residual_matrix(THR2)
    R_ref = oracle.residual_matrix_sym(sc.src, sc.dst, H)
    assert np.array_equal(R.view(np.uint64), R_ref.view(np.uint64))
    assert np.array_equal(cnt, (R_ref < THR2).sum(axis=1))
    assert np.array_equal(engine.score(THR2), cnt)
    assert (R >= R_fwd).all()
    engine.set_residual_mode(False)
    R2, c2 = engine.residual_matrix(THR2)
    assert np.array_equal(R2.view(np.uint64), R_fwd.view(np.uint64)) and np.array_equal(c2, c_fwd)


# ---- epipolar front half on the GPU -------------------------------------
@pytest.fixture(params=[0, 1], ids=["sampson", "epipolar_max"])
def fund_metric(request, engine, oracle):
    """r06: both definitions of the distance to the epipolar geometry (mh_set_fundamental_metric), set on the engine and on
    the oracle for the duration of a test: 0 Sampson, 1 the larger squared point-to-epipolar-line distance — what
    cv::findFundamentalMat thresholds at M/main.cpp:400 and M/MultiH.cpp:775."""
    engine.set_fundamental_metric(request.param)
    oracle.set_fundamental_metric(request.param)
    yield request.param
    oracle.set_fundamental_metric(0)
    engine.set_fundamental_metric(0)


@pytest.mark.parametrize("n,m,seed", [(8, 16, 1), (500, 256, 2), (5000, 2000, 1234)])
def test_fundamental_hypotheses_and_sampson_scores(engine, synth, oracle, n, m, seed, fund_metric):
    sc = synth.make_scene(n, 3, seed=seed, outlier_frac=0.2 if n > 8 else 0.0, with_neighbours=False)
    engine.set_correspondences(sc.src, sc.dst)
    engine.propose_fund8(seed, 3, m)
    F, idx = engine.get_fund_hypotheses()
    assert np.array_equal(idx, oracle.sample8(seed, 3, m, n))
    F_ref = oracle.fund8(sc.src, sc.dst, idx)
    ok = np.isfinite(F_ref).all(axis=1)
    assert ok.mean() > 0.9
    assert np.max(np.abs(F[ok] - F_ref[ok])) <= 1e-6                    # unit Frobenius norm: abs == rel
    assert np.array_equal(F[ok].view(np.uint64), F_ref[ok].view(np.uint64))
    cnt = engine.score_sampson(4.0)
    assert np.array_equal(cnt[ok], oracle.sampson_score(sc.src, sc.dst, F_ref[ok], 4.0))


def test_epipolar_max_is_the_point_to_line_distance(engine, synth, oracle):
    """r06: the second definition against plain numpy — max over the two images of (p2' F p1)^2 / |line normal|^2 — and its
    relation to Sampson's: at least twice it (e^2 / min(A, B) against e^2 / (A + B)), so the same threshold in pixels lets
    fewer correspondences through."""
    sc = synth.make_scene(3000, 3, seed=5, outlier_frac=0.3, with_neighbours=False)
    F = sc.F.reshape(3, 3)
    p1 = np.concatenate([sc.src, np.ones((sc.n, 1))], 1)
    p2 = np.concatenate([sc.dst, np.ones((sc.n, 1))], 1)
    l2, l1 = p1 @ F.T, p2 @ F
    e = np.einsum("ni,ni->n", p2, l2)
    want = np.maximum(e * e / (l2[:, 0] ** 2 + l2[:, 1] ** 2), e * e / (l1[:, 0] ** 2 + l1[:, 1] ** 2))
    oracle.set_fundamental_metric(1)
    try:
        d1 = oracle.sampson(sc.src, sc.dst, sc.F)
    finally:
        oracle.set_fundamental_metric(0)
    d0 = oracle.sampson(sc.src, sc.dst, sc.F)
    assert np.allclose(d1, want, rtol=1e-9, atol=1e-12)
    ok = d0 > 1e-12
    assert (d1[ok] >= 2 * d0[ok] * (1 - 1e-12)).all()
    # the counts of the two definitions at one threshold, engine against oracle, and their order
    engine.set_correspondences(sc.src, sc.dst)
    engine.propose_fund8(11, 0, 256)
    Fh, _ = engine.get_fund_hypotheses()
    counts = {}
    for metric in (0, 1):
        engine.set_fundamental_metric(metric)
        oracle.set_fundamental_metric(metric)
        try:
            counts[metric] = engine.score_sampson(4.0)
            okh = np.isfinite(Fh).all(axis=1)
            assert np.array_equal(counts[metric][okh], oracle.sampson_score(sc.src, sc.dst, Fh[okh], 4.0))
        finally:
            engine.set_fundamental_metric(0)
            oracle.set_fundamental_metric(0)
    assert (counts[1] <= counts[0]).all() and (counts[1] < counts[0]).any()


def test_fundamental_refit_and_estimate(engine, synth, oracle, fund_metric):
    sc = synth.make_scene(5000, 3, seed=1234, with_neighbours=False)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    engine.propose_fund8(99, 0, 1000)
    F, idx = engine.get_fund_hypotheses()
    cnt = engine.score_sampson(4.0)
    best = int(np.argmax(cnt))
    F1, mask, c1 = engine.refit_fundamental(F[best], 4.0, 1)
    F1r, maskr, c1r = oracle.fund_refit(sc.src, sc.dst, F[best], 4.0)
    assert c1 == c1r and np.array_equal(mask, maskr)
    assert np.max(np.abs(F1 - F1r)) <= 1e-6
    assert np.array_equal(F1.view(np.uint64), F1r.view(np.uint64))
    # whole estimate: F close to the scene's true epipolar geometry, epipole where the scene put it
    Fe, e2, m2, inl = engine.estimate_fundamental(99, 1000, 2.0)
    assert inl == int(m2.sum()) and inl > 0.9 * (sc.gt_label >= 0).sum()
    d = oracle.sampson(sc.src[sc.gt_label >= 0], sc.dst[sc.gt_label >= 0], Fe)
    assert np.median(np.sqrt(d)) < 0.5
    assert np.max(np.abs(e2 - sc.e2) / np.abs(sc.e2)) < 0.05
    # and the engine runs its hot loop on the estimated geometry
    engine.set_epipolar(Fe, e2)


def test_process_from_raw_correspondences(mh, engine_lib, synth):
    """Process() without SetEpipolarGeometry: F and the epipole are estimated on the GPU first (the
    reference's GetFundamentalMatrixAndRefineData role), gross outliers are filtered, then the loop runs.
    Also the reference's only real data set end to end with no external geometry at all."""
    import ctypes as C
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    dp = C.POINTER(C.c_double)

    def run(src, dst, aff, thrF):
        n = len(src)
        labels = np.full(n, -7, dtype=np.int32)
        Hout = np.zeros((64, 9))
        it = C.c_int(0)
        src, dst, aff = (np.ascontiguousarray(a) for a in (src, dst, aff))
        k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), n,
                                 None, None, C.c_double(thrF), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5),
                                 20, C.c_ulonglong(1234), 20000, 16, 0, None, 0,
                                 labels.ctypes.data_as(C.POINTER(C.c_int)), Hout.ctypes.data_as(dp), 64,
                                 C.byref(it), None, None, 0, 4)
        return k, labels

    sc = synth.make_scene(5000, 3, seed=1234)
    k, labels = run(sc.src, sc.dst, sc.aff, 2.6)
    assert k >= 3
    kept = int((labels != -7).sum())                       # labels cover the F-filtered points only
    assert 0.7 * sc.n < kept < sc.n
    g = np.load(os.path.join(GOLDEN, "barrsmith.npz"))
    pts = g["points"]
    k, labels = run(pts[:, 0:2], pts[:, 2:4], pts[:, 4:8], 2.6)
    assert 3 <= k <= 8
    kept = labels[labels != -7]
    assert 1000 < kept.size < 2903 and (kept >= 0).sum() > 500


# ---- reference-style initialisation: per-point HAF + mean shift ------------------------------
def test_local_homographies_and_features(engine, synth, oracle):
    sc = synth.make_scene(3000, 3, seed=5, with_neighbours=False)
    _load(engine, sc, neighbours=False)
    H, feat = engine.local_homographies(0.005)
    H_ref, feat_ref = oracle.haf_point(sc.src, sc.dst, sc.aff, sc.F, sc.e2, 0.005)
    ok = np.isfinite(H_ref).all(axis=1)
    assert ok.mean() > 0.99
    assert np.array_equal(H[ok].view(np.uint64), H_ref[ok].view(np.uint64))
    assert np.array_equal(feat[ok].view(np.uint64), feat_ref[ok].view(np.uint64))
    # a point-wise homography maps its own point onto its correspondence (inliers, up to the affinity noise)
    inl = (sc.gt_label >= 0) & ok
    p = np.stack([synth.apply_h(H[i], sc.src[i:i + 1])[0] for i in np.flatnonzero(inl)[:200]])
    assert np.median(np.abs(p - sc.dst[np.flatnonzero(inl)[:200]])) < 1.0


@pytest.mark.parametrize("n,d,seed", [(60, 6, 1), (500, 10, 2), (3000, 10, 3)])
def test_gpu_mean_shift_matches_oracle(engine, oracle, n, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-40, 40, size=(max(3, n // 40), d))
    data = np.concatenate([c + rng.normal(0, 0.2, size=(30, d)) for c in centres])[:n]
    data = np.concatenate([data, rng.uniform(-40, 40, size=(n - len(data), d))]) if len(data) < n else data
    modes, assign, k = engine.mean_shift(data, 2.2, seed)
    modes_o, assign_o, k_o = oracle.mean_shift(data, 2.2, seed)
    assert k == k_o
    assert np.array_equal(assign, assign_o)
    assert np.array_equal(modes.view(np.uint64), modes_o.view(np.uint64))
    assert (assign >= 0).all()


def test_gpu_mean_shift_outside_the_plain_range(engine, oracle):
    """k_ms_partial forms |r| for sqrt(r * r) only where that is exact (2^-500 <= |r| <= 2^500 or r == 0); rows parked at
    1e300 (what EstablishStablePointSets does with a degenerate per-point solve), components that differ by 1e-170 and by
    exactly 0, and a whole cluster scaled to 1e-160 take the reference's form.  Same modes, same assignment."""
    rng = np.random.default_rng(11)
    d = 10
    centres = rng.uniform(-40, 40, size=(12, d))
    data = np.concatenate([c + rng.normal(0, 0.2, size=(30, d)) for c in centres])
    data[5:25] = data[5]                                   # exact duplicates: r == 0 in every component
    data[40:60] = data[40] + rng.uniform(-1e-170, 1e-170, size=(20, d))      # below 2^-500
    data[100:120] = 1e300                                  # parked rows: r * r overflows
    data[200:230] = rng.uniform(-1e-160, 1e-160, size=(30, d))              # a cluster whose own spread underflows when squared
    data[300:305, 3] = -1e300
    modes, assign, k = engine.mean_shift(data, 2.2, 9)
    with np.errstate(all="ignore"):
        modes_o, assign_o, k_o = oracle.mean_shift(data, 2.2, 9)
    assert k == k_o
    assert np.array_equal(assign, assign_o)
    assert np.array_equal(modes.view(np.uint64), modes_o.view(np.uint64))


@pytest.mark.parametrize("d", [6, 10, 7])
def test_gpu_mean_shift_schedules_agree(engine, oracle, d):
    """r05: the tail of a batch of climbs runs in one persistent launch (k_ms_persist: the thread's rows in registers, a
    barrier of the climb's own per iteration; mh_set_tuning key 29 = the number of climbs below which it takes over, 0 =
    a launch per iteration throughout, the r04 schedule).  A schedule, not a result: modes and assignment are the same
    for every setting and equal the oracle's — dense clusters (climbs of dozens of iterations over hundreds of members),
    rows parked at 1e300, and a dimension (7) the persistent form does not exist for."""
    rng = np.random.default_rng(100 + d)
    n = 12000
    centres = rng.uniform(-60, 60, size=(40, d))
    data = np.concatenate([c + rng.normal(0, 0.45, size=(220, d)) for c in centres])
    data = np.concatenate([data, rng.uniform(-60, 60, size=(n - len(data), d))])
    data[7000:7040] = 1e300
    with np.errstate(all="ignore"):
        modes_o, assign_o, k_o = oracle.mean_shift(data, 2.2, 31)
    try:
        # (indexed, persist, per_round): key 32 = climbs through the one-coordinate index, a workgroup each, a launch per
        # batch (the default where it exists: d = 6 / 10); 0 = the launched / persistent schedule of keys 29 and 7
        for indexed, persist, per_round in ((1, 12, 6), (0, 12, 6), (0, 0, 6), (0, 1, 6), (0, 12, 1), (0, 64, 3)):
            engine.set_tuning(32, indexed)
            engine.set_tuning(29, persist)
            engine.set_tuning(7, per_round)
            modes, assign, k = engine.mean_shift(data, 2.2, 31)
            assert k == k_o, (indexed, persist, per_round)
            assert np.array_equal(assign, assign_o), (indexed, persist, per_round)
            assert np.array_equal(modes.view(np.uint64), modes_o.view(np.uint64)), (indexed, persist, per_round)
    finally:
        engine.set_tuning(32, 1)
        engine.set_tuning(29, 12)
        engine.set_tuning(7, 6)


@pytest.mark.parametrize("case", ["one_cell", "wide", "slots", "boundary", "nan", "tiny_band", "split_halves", "dense_walk", "dense_walk_k3"])
def test_gpu_mean_shift_index_edges(engine, oracle, case):
    """r05, k_ms_indexed: the index only narrows where members are LOOKED for.  Inputs that strain that: every row in one
    cell; a spread that takes more cells than the index holds (cells widen, far rows clamp into the last); more rows
    than the 16 384 slots of the definition (a slot sums several rows, in ascending order); rows exactly one band away
    from a seed on the indexed coordinate (in / out by one ulp); NaN coordinates; a band so narrow that every row is its
    own mode.  Modes and assignment equal the oracle's bit for bit."""
    rng = np.random.default_rng(7)
    d, bw, n = 10, 2.2, 3000
    if case == "one_cell":
        data = rng.uniform(0, 3.0, size=(n, d))
    elif case == "wide":
        data = rng.uniform(-40, 40, size=(n, d))
        data[:, 2] = np.concatenate([rng.uniform(-4e6, 4e6, size=n - 600), rng.uniform(0, 3, size=600)])
        data[-600:] = data[-600] + rng.normal(0, 0.3, size=(600, d))
    elif case == "slots":
        n = 40000
        centres = rng.uniform(-30, 30, size=(25, d))
        data = np.concatenate([c + rng.normal(0, 0.4, size=(1200, d)) for c in centres])
        data = np.concatenate([data, rng.uniform(-30, 30, size=(n - len(data), d))])
        data = data[rng.permutation(n)]
    elif case == "boundary":
        data = rng.uniform(-100, 100, size=(n, d))
        band_sq = bw * bw
        for q in range(40):                                   # pairs that differ on ONE coordinate by band^2 -/+ a few ulps
            a = data[10 * q].copy()
            b = a.copy()
            step = band_sq
            for _ in range(q % 5): step = np.nextafter(step, 0.0 if q % 2 else 1e9)
            b[q % d] = a[q % d] + (step if q % 3 else -step)
            data[10 * q + 1] = b
    elif case in ("split_halves", "dense_walk", "dense_walk_k3"):
        # one blob that every climb's ball swallows whole: every group of the definition gets n / 64 members per iteration —
        # 94 (two half-trees of a wave each), 312 and 625 (more than a wave holds: the dense walk over the slots; with
        # 40 000 rows a slot sums three rows) — plus scattered rows; the blob's noise makes the ORDER of the sums show
        n = {"split_halves": 6000, "dense_walk": 20000, "dense_walk_k3": 40000}[case]
        data = rng.uniform(-50, 50, size=(1, d)) + rng.normal(0, 0.05, size=(n, d))
        data[::97] = rng.uniform(-50, 50, size=(len(data[::97]), d))
    elif case == "nan":
        data = rng.uniform(-20, 20, size=(n, d))
        data[5:25, 0] = np.nan
        data[40:50, 3] = np.nan
        data[60:70] = np.inf
        data[80:90, 1] = -1e300
    else:
        bw = 1e-3
        data = rng.uniform(-5, 5, size=(600, d))
    data = np.ascontiguousarray(data)
    with np.errstate(all="ignore"):
        modes_o, assign_o, k_o = oracle.mean_shift(data, bw, 5)
    modes, assign, k = engine.mean_shift(data, bw, 5)
    assert k == k_o
    assert np.array_equal(assign, assign_o)
    assert np.array_equal(modes.view(np.uint64), modes_o.view(np.uint64))


def test_process_with_reference_style_initialisation(mh, engine_lib, synth):
    """INIT_STABLE_SETS: per-point HAF -> mean shift -> 3-point LSQ per cluster (the reference's own
    ComputeLocalHomographies + EstablishStablePointSets), then the usual merge/label loop."""
    import ctypes as C
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    sc = synth.make_scene(3000, 3, seed=77)
    n = sc.n
    dp = C.POINTER(C.c_double)
    labels = np.full(n, -7, dtype=np.int32)
    Hout = np.zeros((256, 9))
    it = C.c_int(0)
    src, dst, aff, F, e2 = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff, sc.F, sc.e2))
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), n,
                             F.ctypes.data_as(dp), e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.2),
                             C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(1234), 0, 0, 0, None, 0,
                             labels.ctypes.data_as(C.POINTER(C.c_int)), Hout.ctypes.data_as(dp), 256,
                             C.byref(it), None, None, 0, -1)
    assert k >= 3 and labels.min() >= -1 and labels.max() < k
    dom = []
    for p in range(3):
        lab_p = labels[sc.gt_label == p]
        vals, counts = np.unique(lab_p[lab_p >= 0], return_counts=True)
        assert counts.max() > 0.5 * (sc.gt_label == p).sum()
        dom.append(int(vals[np.argmax(counts)]))
    assert len(set(dom)) == 3


def test_refine_correspondences(engine, synth, oracle):
    """GetFundamentalMatrixAndRefineData's per-point part (M/MultiH.cpp:807-838) on the GPU vs the oracle:
    keep mask identical, corrected coordinates and optimal affinities bit-identical."""
    sc = synth.make_scene(4000, 3, seed=23, noise=0.5, outlier_frac=0.15, with_neighbours=False)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    e1, e2 = engine.epipoles(sc.F)
    assert np.max(np.abs(e2 - sc.e2) / np.abs(sc.e2)) < 1e-6
    mask = (np.random.default_rng(0).random(sc.n) < 0.9).astype(np.uint8)
    keep, out = engine.refine_correspondences(sc.F, e1, e2, mask)
    keep_o, out_o = oracle.refine_points(sc.src, sc.dst, sc.aff, sc.F, e1, e2, mask)
    assert np.array_equal(keep, keep_o)
    k = keep.astype(bool)
    assert (keep[mask == 0] == 0).all() and k.sum() > 0.6 * sc.n
    assert np.max(np.abs(out[k] - out_o[k]) / np.maximum(1e-12, np.abs(out_o[k]))) <= 1e-6
    assert np.array_equal(out[k].view(np.uint64), out_o[k].view(np.uint64))


def test_process_is_reproducible(mh, engine_lib, synth):
    """Fixed seed -> identical labels, homographies, iteration count and energy on every run (explicit
    counter RNG everywhere the reference uses the unseeded rand(); integer atomics only)."""
    import ctypes as C
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    sc = synth.make_scene(4000, 4, seed=314)
    dp = C.POINTER(C.c_double)
    src, dst, aff = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff))

    def run(init_mode):
        labels = np.full(sc.n, -7, dtype=np.int32)
        Hout = np.zeros((128, 9))
        it, en = C.c_int(0), C.c_double(0)
        k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n,
                                 None, None, C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5),
                                 20, C.c_ulonglong(77), 8000, 16, 0, None, 0,
                                 labels.ctypes.data_as(C.POINTER(C.c_int)), Hout.ctypes.data_as(dp), 128,
                                 C.byref(it), C.byref(en), None, 2000 if init_mode >= 0 else 0, init_mode)
        return k, labels, Hout, it.value, en.value

    for mode in (4, -1):                      # DLT proposals with re-proposal; reference-style initialisation
        a = run(mode)
        b = run(mode)
        assert a[0] == b[0] >= 2 and a[3] == b[3] and a[4] == b[4]
        assert np.array_equal(a[1], b[1])
        assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
