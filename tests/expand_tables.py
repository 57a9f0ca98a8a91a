"""Alpha-expansion problems that do not come from a scene: arbitrary non-negative int32 cost tables and hand-built
neighbour graphs, for the CPU references (oracle.expand, the reference's compiled GCO) and for the engine.

GCO's contract, and so mh_expand's, is any non-negative int32 table (GCoptimization.cpp:975-1289).  The scene-derived costs of
mh_data_cost have a narrow structure (one outlier cost per scene, a few lambdas, edge weights of round(100 lambda) x
multiplicity); the families here leave it: ties across many labels, per-site outlier costs, duplicate and dead columns, Potts
weights from 0 to 10^6, hubs, long chains, cliques, isolated sites, heavy multiplicity, terms near the int32 bounds.

A problem is (cost [n, L] int32, site-major; hit_rowptr, hit_col: DIRECTED hit lists as mh_set_neighbors_csr takes them — self
hits and duplicates allowed, the symmetric multiplicity is the weight; potts; initial labeling or None = all zero).

load_into_engine() gives the engine such a problem through its public entry points only: mh_data_cost sizes and marks the cost
buffer, which is then overwritten on the device (MH_BUF_COST) by a hipMemcpy of the HIP runtime the engine has loaded.
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
import zlib
from dataclasses import dataclass

import numpy as np

INT32_MAX = 0x7fffffff
MH_BUF_COST = 4


@dataclass
class Problem:
    name: str
    cost: np.ndarray            # [n, L] int32
    rowptr: np.ndarray          # [n + 1] int32
    col: np.ndarray             # [nnz] int32
    potts: int
    init: np.ndarray | None = None

    @property
    def n(self):
        return self.cost.shape[0]

    @property
    def L(self):
        return self.cost.shape[1]


# ---- graphs (directed hit lists) -----------------------------------------------------------------------------------------

def csr(n, rows, cols):
    """Directed hits (rows[k] -> cols[k]) as a CSR, the hits of a row in the order given."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    rp = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return rp, cols[order].astype(np.int32)


def graph_none(n):
    return np.zeros(n + 1, np.int32), np.zeros(0, np.int32)


def graph_path(n):
    i = np.arange(n - 1)
    return csr(n, i, i + 1)


def graph_star(n, hub=0):
    """A hub hit by every other site (degree n - 1 in the symmetric graph)."""
    others = np.array([i for i in range(n) if i != hub], dtype=np.int64)
    return csr(n, others, np.full(others.size, hub))


def graph_clique_isolated(n, k=200):
    """A clique on the first k sites (one directed hit per pair), the rest isolated."""
    a, b = np.triu_indices(min(k, n), 1)
    return csr(n, a, b)


def graph_random_multi(n, rng, deg=6, self_hits=0.05, dup_hits=0.2):
    """Random directed hits with self hits and duplicated hits (multiplicity > 1, and hits both ways)."""
    rows = np.repeat(np.arange(n), deg)
    cols = rng.integers(0, n, size=rows.size)
    ns, nd = int(self_hits * rows.size), int(dup_hits * rows.size)
    si = rng.integers(0, n, size=ns)
    di = rng.integers(0, rows.size, size=nd)
    rows = np.concatenate([rows, si, rows[di], cols[di]])
    cols = np.concatenate([cols, si, cols[di], rows[di]])
    return csr(n, rows, cols)


def graph_components(n, rng, parts=5):
    """Disconnected random components (sites of a component share a contiguous index range)."""
    cuts = np.sort(rng.choice(np.arange(1, n), size=min(parts - 1, n - 1), replace=False)) if n > 1 else np.zeros(0, int)
    bounds = np.concatenate([[0], cuts, [n]])
    rows, cols = [], []
    for a, b in zip(bounds[:-1], bounds[1:]):
        m = b - a
        if m < 2:
            continue
        r = np.repeat(np.arange(a, b), 3)
        rows.append(r)
        cols.append(rng.integers(a, b, size=r.size))
    if not rows:
        return graph_none(n)
    return csr(n, np.concatenate(rows), np.concatenate(cols))


def graph_heavy(n, rng, mult=40):
    """A sparse random graph whose every hit is repeated `mult` times (heavy multiplicity weights)."""
    rows = np.repeat(np.arange(n), 2)
    cols = rng.integers(0, n, size=rows.size)
    return csr(n, np.repeat(rows, mult), np.repeat(cols, mult))


# ---- cost tables ---------------------------------------------------------------------------------------------------------

def costs_ties(rng, n, L, c):
    return rng.integers(0, c + 1, size=(n, L)).astype(np.int32)


def costs_outlier_per_site(rng, n, L, lam_inv=200):
    """dataEnergy-shaped: column 0 (the outlier label) varies by site; every other entry is in [0, lam_inv] or exactly twice
    that site's outlier cost."""
    c0 = rng.integers(lam_inv // 2, 4 * lam_inv, size=n)
    cost = rng.integers(0, lam_inv + 1, size=(n, L)).astype(np.int64)
    far = rng.random((n, L)) < 0.6
    cost[far] = (2 * c0[:, None] * np.ones((1, L), np.int64))[far]
    cost[:, 0] = c0
    return cost.astype(np.int32)


def costs_duplicate_dead(rng, n, L, kind):
    """kind 'dup': columns 1 and 2 (and the last two) are copies of each other and cheaper than the rest, so consecutive moves
    touch the same sites; 'dead': one column no site prefers (its moves are idempotent); 'all': one column every site prefers."""
    cost = rng.integers(100, 400, size=(n, L)).astype(np.int32)
    if kind == "dup":
        cost[:, 1] = rng.integers(0, 60, size=n)
        cost[:, min(2, L - 1)] = cost[:, 1]
        if L >= 5:
            cost[:, L - 1] = rng.integers(0, 90, size=n)
            cost[:, L - 2] = cost[:, L - 1]
    elif kind == "dead":
        cost[:, L // 2] = 1_000_000
    elif kind == "all":
        cost[:, L // 2] = rng.integers(0, 20, size=n)
    return cost


def costs_alternating(n, L, lo=0, hi=300):
    """Site i prefers label 1 + i % 2 (of labels >= 1), strongly: long augmenting paths along a chain."""
    cost = np.full((n, L), hi, dtype=np.int32)
    i = np.arange(n)
    cost[i, 1 + (i % 2) % (L - 1)] = lo
    cost[:, 0] = hi // 2 + 1
    return cost


def init_labels(rng, n, L, kind):
    if kind == "none":
        return None
    if kind == "random":
        return rng.integers(0, L, size=n).astype(np.int32)
    if kind == "last":
        return np.full(n, L - 1, np.int32)
    raise ValueError(kind)


# ---- energies, exact -----------------------------------------------------------------------------------------------------

def sym_edges(n, rowptr, col):
    """The symmetric weighted graph of directed hits (self hits dropped, multiplicities summed): (i, j, w) with i < j."""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    cols = np.asarray(col, dtype=np.int64)
    keep = rows != cols
    a, b = np.minimum(rows[keep], cols[keep]), np.maximum(rows[keep], cols[keep])
    if a.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    key, w = np.unique(a * n + b, return_counts=True)
    return key // n, key % n, w.astype(np.int64)


def energy_int(cost, rowptr, col, potts, labels):
    """The GCO energy of a labeling in exact Python integers."""
    n = cost.shape[0]
    lab = [int(x) for x in labels]
    e = sum(int(cost[i, lab[i]]) for i in range(n))
    a, b, w = sym_edges(n, rowptr, col)
    e += int(potts) * sum(int(wk) for ia, ib, wk in zip(a.tolist(), b.tolist(), w.tolist()) if lab[ia] != lab[ib])
    return e


def energy_np(cost, rowptr, col, potts, labels):
    """The same in int64 numpy (what the GPU tests recompute the engine's labeling with)."""
    n = cost.shape[0]
    labels = np.asarray(labels, dtype=np.int64)
    a, b, w = sym_edges(n, rowptr, col)
    data = np.asarray(cost, dtype=np.int64)[np.arange(n), labels].sum()
    return int(data + np.int64(potts) * (w * (labels[a] != labels[b])).sum())


def best_expansion_move(cost, rowptr, col, potts, labels):
    """Brute force: the lowest energy over EVERY alpha-expansion move of `labels` (every alpha, every subset of the sites not
    labelled alpha switching to it), with the alpha that reaches it.  Exact integers (int64 on values far below 2^62, checked)."""
    cost = np.asarray(cost, dtype=np.int64)
    n, L = cost.shape
    assert n <= 16 and int(cost.max(initial=0)) < (1 << 40) and potts < (1 << 40)
    a, b, w = sym_edges(n, rowptr, col)
    base = np.asarray(labels, dtype=np.int64)
    masks = np.arange(1 << n, dtype=np.int64)
    bits = (masks[:, None] >> np.arange(n)) & 1                       # [2^n, n]
    best = (energy_int(cost, rowptr, col, potts, base), -1)
    for alpha in range(L):
        free = base != alpha
        sel = bits.astype(bool) & free[None, :]
        lab = np.where(sel, alpha, base[None, :])                       # [2^n, n]
        e = cost[np.arange(n)[None, :], lab].sum(axis=1)
        if a.size:
            e = e + potts * ((lab[:, a] != lab[:, b]) * w[None, :]).sum(axis=1)
        k = int(np.argmin(e))
        if int(e[k]) < best[0]:
            best = (int(e[k]), alpha)
    return best


# ---- families ------------------------------------------------------------------------------------------------------------

def _graph(kind, n, rng):
    if kind == "none":
        return graph_none(n)
    if kind == "path":
        return graph_path(n)
    if kind == "star":
        return graph_star(n)
    if kind == "clique":
        return graph_clique_isolated(n)
    if kind == "multi":
        return graph_random_multi(n, rng)
    if kind == "components":
        return graph_components(n, rng)
    if kind == "heavy":
        return graph_heavy(n, rng)
    raise ValueError(kind)


def problem(family, n, L, graph, potts=50, init="none", seed=0, **kw):
    """One seeded problem of a family (see the module's header)."""
    rng = np.random.default_rng([seed, n, L, zlib.crc32(family.encode()), zlib.crc32(graph.encode())])
    if family == "ties":
        cost = costs_ties(rng, n, L, kw.get("c", 3))
    elif family == "outlier":
        cost = costs_outlier_per_site(rng, n, L)
    elif family in ("dup", "dead", "all"):
        cost = costs_duplicate_dead(rng, n, L, family)
    elif family == "alternating":
        cost = costs_alternating(n, L)
    else:
        raise ValueError(family)
    rp, col = _graph(graph, n, rng)
    name = f"{family}{kw.get('c', '')}-{graph}-n{n}-L{L}-p{potts}-{init}-s{seed}"
    return Problem(name, cost, rp, col, int(potts), init_labels(rng, n, L, init))


def scaled(p: Problem, cost_scale=1, cost_add=0, potts=None, name=None):
    """A problem's table scaled towards the int32 bounds (values are checked to stay int32)."""
    c = p.cost.astype(np.int64) * int(cost_scale) + int(cost_add)
    assert c.min() >= 0 and c.max() <= INT32_MAX
    return Problem(name or p.name + f"-x{cost_scale}+{cost_add}", c.astype(np.int32), p.rowptr, p.col,
                   p.potts if potts is None else int(potts), p.init)


def tiny_problems(count=60, seed=0):
    """Problems small enough for best_expansion_move: n <= 12, L <= 4, every family and graph kind."""
    out = []
    rng = np.random.default_rng(seed)
    fams = [("ties", {"c": 1}), ("ties", {"c": 3}), ("ties", {"c": 255}), ("outlier", {}), ("dup", {}), ("dead", {}),
            ("all", {})]
    graphs = ["none", "path", "star", "clique", "multi", "components", "heavy"]
    pottses = [0, 1, 7, 50, 1000]
    for k in range(count):
        fam, kw = fams[k % len(fams)]
        n = int(rng.integers(1, 13))
        L = int(rng.integers(2, 5))
        if fam in ("dup", "dead", "all") and L < 3:
            L = 3
        g = graphs[(k // len(fams)) % len(graphs)]
        pv = pottses[int(rng.integers(0, len(pottses)))]
        init = ("none", "random", "last")[k % 3]
        out.append(problem(fam, n, L, g, potts=pv, init=init, seed=seed * 1000 + k, **kw))
    return out


# ---- the engine ----------------------------------------------------------------------------------------------------------

_hip = None


def _hip_runtime():
    """The HIP runtime the engine library is linked against (dlopen returns the already-loaded copy)."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    return _hip


def lam_for_potts(potts):
    """A lambda with round(100 lambda) == potts (lambda must be positive: potts 0 takes 0.001)."""
    lam = potts / 100.0 if potts > 0 else 0.001
    assert int(round(100.0 * lam)) == potts
    return lam


def load_into_engine(e, p: Problem):
    """Give the engine `p`: parameters (their Potts weight), n dummy correspondences, L - 1 dummy models, the data cost
    computed (which sizes the cost buffer and marks it current), then overwritten with p.cost; the graph last."""
    n, L = p.cost.shape
    e.set_params(3.0, 2.5, 0.002, lam_for_potts(p.potts), 0)          # first: it marks the data cost stale
    pts = np.stack([np.arange(n, dtype=np.float64) % 997, np.arange(n, dtype=np.float64) // 997], axis=1)
    e.set_correspondences(pts, pts)
    e.set_models(np.tile(np.eye(3).reshape(1, 9), (L - 1, 1)))
    e.data_cost(fetch=False)
    ptr, nbytes = e.device_buffer(MH_BUF_COST)
    assert nbytes >= 4 * n * L, (nbytes, n, L)
    e.synchronize()
    cost = np.ascontiguousarray(p.cost, dtype=np.int32)
    rc = _hip_runtime().hipMemcpy(C.c_void_p(ptr), cost.ctypes.data_as(C.c_void_p), 4 * n * L, 1)   # hipMemcpyHostToDevice
    assert rc == 0, f"hipMemcpy failed ({rc})"
    e.set_neighbors_csr(p.rowptr, p.col)
    # the table is what the engine now holds
    back = np.empty((n, L), np.int32)
    rc = _hip_runtime().hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), 4 * n * L, 2)  # hipMemcpyDeviceToHost
    assert rc == 0 and np.array_equal(back, cost)


def class_s_schedules(seed, count=3, n=0):
    """`count` seeded combinations of the class-S keys of the solver (none changes a result), as {key: value}.  Two solver
    workgroups (key 5) hold about 10 000 sites in their LDS rows (beyond, mh_expand refuses with MH_ERR_INVALID): larger
    problems take 32 there."""
    choices = {5: (256, 32, 2), 6: (0, 2), 11: (0, 1), 12: (1, 2), 17: (0, 2), 37: (1, 2, 16), 38: (0, 16), 39: (0, 16, 64)}
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        s = {k: v[int(rng.integers(0, len(v)))] for k, v in choices.items()}
        if n > 8000 and s[5] == 2:
            s[5] = 32
        out.append(s)
    return out


SCHEDULE_DEFAULTS = {5: 256, 6: 2, 11: 1, 12: 1, 17: 2, 37: 16, 38: 16, 39: 0}


def gco_neighbour_entries_fit(p: Problem):
    """Whether the reference's GCO can take p's graph: GCoptimizationGeneralGraph::finalizeNeighbors
    (GCoptimization.cpp:1587-1612) gathers a site's neighbour entries — one per directed hit at either end, duplicates
    included — into scratch arrays of n entries, so a site with more than n entries overruns the heap there.  The engine and
    the oracle merge duplicates into weights and have no such limit."""
    n = p.n
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(p.rowptr))
    cols = np.asarray(p.col, dtype=np.int64)
    keep = rows != cols
    cnt = np.bincount(rows[keep], minlength=n) + np.bincount(cols[keep], minlength=n)
    return bool(cnt.max(initial=0) <= n)


def initial_energy_fits(p: Problem):
    """Whether the energy of p's initial labeling fits GCO's int32 EnergyType.  When it does not, GCO compares wrapped
    energies (GCoptimization.cpp:1036, 1259) and its result is not a minimiser of anything; the engine refuses such a call
    (MH_ERR_OVERFLOW)."""
    lab = np.zeros(p.n, np.int32) if p.init is None else p.init
    return energy_int(p.cost, p.rowptr, p.col, p.potts, lab) <= INT32_MAX
