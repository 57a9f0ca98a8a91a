"""mh_expand on arbitrary cost tables and hand-built graphs (tests/expand_tables.py), against the reference's compiled GCO
(labels, energy), the oracle (cycle counts), an int64 recomputation of the returned labeling's energy and, for tiny problems, a
brute force over every expansion move.  Every case runs under the default schedule and seeded combinations of the class-S keys
of the solver (none changes a result).  Also: the overflow contract of mh_expand's header, and the test hook of key 40 (a solve
marked failed) in a move its batch keeps and in one it throws away."""
import numpy as np
import pytest

import expand_tables as X

pytestmark = pytest.mark.gpu

MH_ERR_HIP, MH_ERR_OVERFLOW = -3, -5
FAMILIES = [("ties", {"c": 1}), ("ties", {"c": 3}), ("ties", {"c": 255}), ("ties", {"c": 100000}), ("outlier", {}),
            ("dup", {}), ("dead", {}), ("all", {})]
GRAPHS = ["none", "path", "star", "clique", "multi", "components", "heavy"]
POTTS = [0, 1, 50, 10**6]
INITS = ["none", "random", "last"]


@pytest.fixture
def restore(engine):
    yield
    for k, v in X.SCHEDULE_DEFAULTS.items():
        engine.set_tuning(k, v)
    engine.set_tuning(40, 0)


def _reference(oracle, p):
    """GCO's labels and energy (the oracle's restatement where the reference build is absent: the CPU suite holds them equal on
    these families) and the oracle's cycle count."""
    lab_o, e_o, cyc_o, _ = oracle.expand(p.cost, p.rowptr, p.col, p.potts, init_labels=p.init)
    if oracle.ref() is not None and X.gco_neighbour_entries_fit(p):
        lab_r, e_r = oracle.ref_expand_table(p.cost, p.rowptr, p.col, p.potts, init_labels=p.init)
        assert e_r == e_o and np.array_equal(lab_r, lab_o), p.name
    return lab_o, e_o, cyc_o


def _run(engine, p):
    X.load_into_engine(engine, p)
    return engine.expand(p.init)


def _check(engine, oracle, p, schedules=3, seed=0):
    lab_r, e_r, cyc_r = _reference(oracle, p)
    for sched in [{}] + X.class_s_schedules(seed, schedules, p.n):
        for k, v in X.SCHEDULE_DEFAULTS.items():
            engine.set_tuning(k, sched.get(k, v))
        lab, e, cyc = _run(engine, p)
        where = (p.name, sched)
        assert e == e_r, where
        assert np.array_equal(lab, lab_r), (where, int((lab != lab_r).sum()))
        assert cyc == cyc_r, where
        assert X.energy_np(p.cost, p.rowptr, p.col, p.potts, lab) == e, where
        st = engine.expand_stats()
        assert st["barrier_timeout_retries"] == 0, where


def _family_cases():
    out = []
    for fi, (fam, kw) in enumerate(FAMILIES):
        for gi, g in enumerate(GRAPHS):
            pv = POTTS[(fi + gi) % len(POTTS)]
            init = INITS[(fi + 2 * gi) % len(INITS)] if pv < 10**6 else "last"
            out.append((fam, kw, g, pv, init))
    return out


@pytest.mark.parametrize("fam,kw,graph,potts,init", _family_cases(),
                         ids=[f"{f}{kw.get('c', '')}-{g}-p{p}-{i}" for f, kw, g, p, i in _family_cases()])
def test_families(engine, oracle, restore, fam, kw, graph, potts, init):
    p = X.problem(fam, 1000, 17, graph, potts=potts, init=init, seed=1, **kw)
    _check(engine, oracle, p, seed=len(p.name))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4097, 20011])
def test_shapes(engine, oracle, restore, n):
    """Wave edges (16 / 32 / 64 sites per wave of key 39) and label counts below, at and one beyond a batch of 16."""
    Ls = [2, 3, 16, 17, 33] + ([300] if n <= 1000 else [])
    for k, L in enumerate(Ls):
        fam, g, init = [("ties", "multi", "random"), ("outlier", "components", "none"), ("dup", "path", "last")][k % 3]
        p = X.problem(fam, n, L, g, potts=(7, 50, 1)[k % 3], init=init, seed=5, c=3)
        _check(engine, oracle, p, schedules=2, seed=n + L)


def test_long_chain_star_clique(engine, oracle, restore):
    for p in (X.problem("alternating", 20000, 3, "path", potts=50, seed=1),
              X.problem("alternating", 20000, 3, "path", potts=200, seed=1),
              X.problem("ties", 4097, 16, "star", potts=3, init="random", seed=4, c=255),
              X.problem("outlier", 2000, 17, "clique", potts=1, init="random", seed=4),
              X.problem("dup", 3000, 33, "heavy", potts=2, init="random", seed=4)):
        _check(engine, oracle, p, seed=p.n)


def test_tiny_brute_force(engine, oracle, restore):
    """n <= 12, L <= 4: the engine's result is the oracle's, and no alpha-expansion move lowers its energy (exact integers)."""
    for p in X.tiny_problems(60, seed=7):
        lab, e, cyc = _run(engine, p)
        lab_r, e_r, cyc_r = _reference(oracle, p)
        assert e == e_r and np.array_equal(lab, lab_r) and cyc == cyc_r, p.name
        assert X.energy_int(p.cost, p.rowptr, p.col, p.potts, lab) == e
        best, alpha = X.best_expansion_move(p.cost, p.rowptr, p.col, p.potts, lab)
        assert best == e and alpha == -1, (p.name, best, alpha)


def _expect_overflow(engine, p):
    with pytest.raises(Exception) as ei:
        _run(engine, p)
    assert getattr(ei.value, "code", None) == MH_ERR_OVERFLOW, (p.name, str(ei.value))


def test_overflow_contract(engine, oracle, restore):
    """Below the bound of mh_expand's header the result is GCO's; above it the call is refused with MH_ERR_OVERFLOW (never
    MH_OK with another labeling), and the same engine then solves the next table."""
    rng = np.random.default_rng(11)
    ok = X.problem("ties", 3000, 5, "multi", potts=50, init="random", seed=11, c=255)
    # just below: an initial energy of 2^30 - small, every term large
    base = X.problem("ties", 64, 3, "path", potts=1, init="last", seed=12, c=255)
    E0 = X.energy_int(base.cost, base.rowptr, base.col, base.potts, base.init)
    s = (1 << 30) // (E0 + 1)
    below = X.scaled(base, cost_scale=s, potts=s, name="below-2^30")
    assert X.energy_int(below.cost, below.rowptr, below.col, below.potts, below.init) <= 1 << 30
    _check(engine, oracle, below, schedules=1)
    # above: the initial labeling's energy exceeds int32 (two sites of 2^30 + 1 each on the start label) ...
    n = 2000
    cost = rng.integers(0, 100, size=(n, 4)).astype(np.int32)
    cost[:2, 3] = (1 << 30) + 1
    rp, col = X.graph_path(n)
    above = X.Problem("initial-energy-above-int32", cost, rp, col, 5, np.full(n, 3, np.int32))
    assert not X.initial_energy_fits(above)
    for sched in [{}] + X.class_s_schedules(13, 2):
        for k, v in X.SCHEDULE_DEFAULTS.items():
            engine.set_tuning(k, sched.get(k, v))
        _expect_overflow(engine, above)
        _check(engine, oracle, ok, schedules=0)
    # ... one n-link potts * w beyond int32 (2200 hits between two sites, potts 10^6; the energy itself stays small)
    rows = np.concatenate([np.zeros(1100, np.int64), np.ones(1100, np.int64), np.arange(2, n - 1)])
    cols = np.concatenate([np.ones(1100, np.int64), np.zeros(1100, np.int64), np.arange(3, n)])
    rp, col = X.csr(n, rows, cols)
    cost = rng.integers(0, 100, size=(n, 4)).astype(np.int32)
    heavy = X.Problem("nlink-above-int32", cost, rp, col, 10**6, None)
    assert X.initial_energy_fits(heavy)
    _expect_overflow(engine, heavy)
    _check(engine, oracle, ok, schedules=0)
    # between 2^30 and 2^31 the solver may refuse (the deviation in the header) but never returns another result
    cost = np.zeros((n, 3), np.int32)
    cost[0, 0] = (1 << 30) + 5
    cost[1, 1] = (1 << 30) + 5
    cost[2:, 0] = rng.integers(0, 50, size=n - 2)
    rp, col = X.graph_path(n)
    mid = X.Problem("terms-between-2^30-and-2^31", cost, rp, col, 1 << 20, None)
    lab_r, e_r, cyc_r = _reference(oracle, mid)
    try:
        lab, e, cyc = _run(engine, mid)
        assert e == e_r and np.array_equal(lab, lab_r) and cyc == cyc_r
    except Exception as ex:                                                  # noqa: BLE001
        assert getattr(ex, "code", None) == MH_ERR_OVERFLOW, str(ex)
    _check(engine, oracle, ok, schedules=0)


def _dup_table():
    """Columns 0 and 1 identical and far cheaper than the start label: move 0 (context 0 of the first batch) is accepted and
    changes every site, so move 1 — solved beside it on the old labeling — fails its test and is thrown away."""
    n, L = 2000, 17
    rng = np.random.default_rng(21)
    cost = rng.integers(200, 400, size=(n, L)).astype(np.int32)
    cost[:, 0] = rng.integers(0, 50, size=n)
    cost[:, 1] = cost[:, 0]
    rp, col = X.graph_random_multi(n, rng, deg=4)
    return X.Problem("dup-columns-0-1", cost, rp, col, 3, np.full(n, L - 1, np.int32))


def test_injected_failure_in_an_invalidated_context(engine, oracle, restore):
    """A solve that fails in a context its batch throws away (an accepted predecessor changed the labeling) was never posed by
    the sequential order: the expansion must finish with GCO's result, without a restart."""
    p = _dup_table()
    lab_r, e_r, cyc_r = _reference(oracle, p)
    lab, e, cyc = _run(engine, p)                      # without the hook: the batch's first test fails at move 1
    assert e == e_r and np.array_equal(lab, lab_r)
    assert engine.expand_batch_stats()["batch_invalid"] >= 1
    for ctx in (1, 2, 9):
        engine.set_tuning(40, (1 << 4) | ctx)          # the first group of moves (the first batch), context ctx
        lab, e, cyc = _run(engine, p)
        assert e == e_r and np.array_equal(lab, lab_r) and cyc == cyc_r, ctx
        bs = engine.expand_batch_stats()
        assert bs["batch_invalid"] >= 1 and bs["injected_discarded"] == 1, (ctx, bs)    # word 5: the injected failure was thrown away
        assert engine.expand_stats()["barrier_timeout_retries"] == 0


def test_injected_failure_without_an_accepted_predecessor(engine, oracle, restore):
    """A kept move whose solve fails ends the call with the solver's error; the next call succeeds."""
    p = _dup_table()
    lab_r, e_r, cyc_r = _reference(oracle, p)
    for moves_per_batch, value in ((16, (1 << 4) | 0), (1, (3 << 4) | 0)):
        engine.set_tuning(37, moves_per_batch)
        engine.set_tuning(40, value)
        with pytest.raises(Exception) as ei:
            _run(engine, p)
        assert getattr(ei.value, "code", None) == MH_ERR_HIP and "did not converge" in str(ei.value), str(ei.value)
        lab, e, cyc = _run(engine, p)
        assert e == e_r and np.array_equal(lab, lab_r) and cyc == cyc_r
