"""CPU tests of the alpha-expansion on arbitrary cost tables and hand-built graphs (tests/expand_tables.py): the oracle's
restatement against the reference's compiled GCO, and both against a brute force over every expansion move of tiny problems
(exact integers; no solver involved)."""
import numpy as np
import pytest

import expand_tables as X

FAMILIES = [("ties", {"c": 1}), ("ties", {"c": 3}), ("ties", {"c": 255}), ("ties", {"c": 100000}), ("outlier", {}),
            ("dup", {}), ("dead", {}), ("all", {})]
GRAPHS = ["none", "path", "star", "clique", "multi", "components", "heavy"]
POTTS = [0, 1, 50, 10**6]
INITS = ["none", "random", "last"]


def _need_ref(oracle):
    if oracle.ref() is None:
        pytest.skip("oracle/_ref/libmh_ref_gco.so not built (needs the reference's sources)")


def _family_cases():
    out = []
    for fi, (fam, kw) in enumerate(FAMILIES):
        for gi, g in enumerate(GRAPHS):
            pv = POTTS[(fi + gi) % len(POTTS)]
            init = INITS[(fi + 2 * gi) % len(INITS)] if pv < 10**6 else "last"    # (a random start at 10^6 overflows)
            out.append((fam, kw, g, pv, init))
    return out


def _check_vs_ref(oracle, p):
    lab, e, cyc, en = oracle.expand(p.cost, p.rowptr, p.col, p.potts, init_labels=p.init)
    lab_r, e_r = oracle.ref_expand_table(p.cost, p.rowptr, p.col, p.potts, init_labels=p.init)
    assert e == e_r, p.name
    assert np.array_equal(lab, lab_r), (p.name, int((lab != lab_r).sum()))
    assert X.energy_np(p.cost, p.rowptr, p.col, p.potts, lab) == e
    assert all(en[i + 1] <= en[i] for i in range(len(en) - 1))
    return lab, e, cyc


@pytest.mark.parametrize("fam,kw,graph,potts,init", _family_cases(),
                         ids=[f"{f}{kw.get('c', '')}-{g}-p{p}-{i}" for f, kw, g, p, i in _family_cases()])
def test_oracle_vs_gco_families(oracle, fam, kw, graph, potts, init):
    _need_ref(oracle)
    p = X.problem(fam, 1000, 17, graph, potts=potts, init=init, seed=1, **kw)
    assert X.gco_neighbour_entries_fit(p) and X.initial_energy_fits(p)
    _check_vs_ref(oracle, p)


@pytest.mark.parametrize("potts", POTTS)
def test_oracle_vs_gco_potts_weights(oracle, potts):
    """Every Potts weight on the same tables and graphs; at 10^6 the smoothness term dominates and tie-breaking decides the
    one label everything ends on."""
    _need_ref(oracle)
    for g in ("path", "multi", "clique"):
        for fam, kw in (("ties", {"c": 255}), ("dup", {})):
            p = X.problem(fam, 400, 5, g, potts=potts, init="last", seed=2, **kw)
            assert X.initial_energy_fits(p)
            lab, e, _ = _check_vs_ref(oracle, p)
            if potts == 10**6 and g != "clique":       # (the clique's isolated sites keep their own minima)
                assert np.unique(lab).size == 1


@pytest.mark.parametrize("n,L", [(1, 2), (2, 3), (63, 16), (64, 17), (65, 33), (1000, 300), (4097, 17), (20011, 3)])
def test_oracle_vs_gco_shapes(oracle, n, L):
    _need_ref(oracle)
    for k, (fam, g, init) in enumerate([("ties", "multi", "random"), ("outlier", "components", "none"),
                                        ("dup", "path", "last")]):
        p = X.problem(fam, n, L, g, potts=(7, 50, 1)[k], init=init, seed=3, c=3)
        if not X.gco_neighbour_entries_fit(p):      # (n = 1, 2 with duplicated hits: more entries than sites)
            continue
        _check_vs_ref(oracle, p)


def test_oracle_vs_gco_long_chain(oracle):
    """A path of 20 000 sites with alternating preferences: long augmenting paths, many relabel rounds."""
    _need_ref(oracle)
    for pv in (50, 200):
        p = X.problem("alternating", 20000, 3, "path", potts=pv, seed=1)
        _check_vs_ref(oracle, p)


def test_oracle_vs_gco_star_hub(oracle):
    _need_ref(oracle)
    p = X.problem("ties", 4097, 16, "star", potts=3, init="random", seed=4, c=255)
    _check_vs_ref(oracle, p)


def test_gco_wraps_an_initial_energy_beyond_int32(oracle):
    """A finding of these families: when the initial labeling's energy exceeds int32, GCO compares wrapped energies and its
    result differs from the oracle's (which sums in int64).  Such calls are outside the contract: the engine refuses them
    (MH_ERR_OVERFLOW; tests/test_gpu_expand_tables.py)."""
    _need_ref(oracle)
    p = X.problem("ties", 1000, 17, "multi", potts=10**6, init="random", seed=1, c=1)
    assert not X.initial_energy_fits(p)
    lab, e, _, _ = oracle.expand(p.cost, p.rowptr, p.col, p.potts, init_labels=p.init)
    lab_r, e_r = oracle.ref_expand_table(p.cost, p.rowptr, p.col, p.potts, init_labels=p.init)
    assert e_r < 0 and e >= 0 and not np.array_equal(lab, lab_r)


def test_gco_neighbour_entry_limit():
    """The reference's finalizeNeighbors holds a site's neighbour entries in n-entry scratch arrays; the families above keep to
    that limit wherever they are compared with it (a heavy-multiplicity graph on few sites does not)."""
    p = X.problem("ties", 4, 3, "heavy", potts=1, seed=0, c=1)
    assert not X.gco_neighbour_entries_fit(p)
    assert X.gco_neighbour_entries_fit(X.problem("ties", 1000, 3, "heavy", potts=1, seed=0, c=1))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_tiny_no_expansion_move_lowers_the_energy(oracle, seed):
    """Independent of GCO and of the oracle's solver: for n <= 12, L <= 4, enumerate every alpha-expansion move of the result
    and assert that none lowers its energy (exact integers); the oracle's energy is the labeling's, and it equals GCO's result
    wherever GCO can take the graph."""
    for p in X.tiny_problems(40, seed=seed):
        lab, e, _, _ = oracle.expand(p.cost, p.rowptr, p.col, p.potts, init_labels=p.init)
        assert X.energy_int(p.cost, p.rowptr, p.col, p.potts, lab) == e, p.name
        best, alpha = X.best_expansion_move(p.cost, p.rowptr, p.col, p.potts, lab)
        assert best == e and alpha == -1, (p.name, best, alpha, e)
        if oracle.ref() is not None and X.gco_neighbour_entries_fit(p):
            lab_r, e_r = oracle.ref_expand_table(p.cost, p.rowptr, p.col, p.potts, init_labels=p.init)
            assert e_r == e and np.array_equal(lab_r, lab), p.name
