"""The label cost without a GPU: the twin's contract (tests/label_cost_numpy.py: the energy of the labeling with alt in place of k,
minus the energy before, is drop_delta's delta — for every label of a 4-label case under both data terms and both errors), the tie
rule of the best alternative, sites without a candidate, a label that neighbours only itself, the host's rule and bookkeeping
(host/merge_step.cpp through mhh_select_merges_label_cost, mhh_select_drop, mhh_apply_drop) against the twin's, the new exports and
weak references, the harness flag, and the new kernels' resource report."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import data_term_numpy as T
import label_cost_numpy as L
import merge_energy_numpy as M
import oracle_lib as O
import refit_h_numpy as R

LAM, THR2 = 0.5, 2.2 ** 2
OUTLIER = T.outlier_cost(LAM, THR2)
_cache = {}
_ip, _lp, _dp = C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def host(mh, engine_lib):
    lib = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    assert hasattr(lib, "mhh_select_merges_label_cost") and hasattr(lib, "mhh_select_drop") and hasattr(lib, "mhh_apply_drop")
    return lib


def _case():
    """360 points on four noisy planes with near-true models (two of them of nearly one plane), a labeling with outliers and wrong
    labels, and directed hit lists with one-way hits (w = 1), mutual hits (w = 2), self hits and an isolated site.  Once."""
    if "case" in _cache:
        return _cache["case"]
    rng = np.random.default_rng(7)
    n, nh = 360, 4
    truth = rng.integers(0, nh, size=n)
    src, dst = np.empty((n, 2)), np.empty((n, 2))
    H = np.empty((nh, 9))
    for k in range(nh):
        m = truth == k
        s, d, Hk, _ = R.plane_scene(rng, int(m.sum()), 0.7)
        src[m], dst[m], H[k] = s, d, Hk
    H[1] = H[0] * (1.0 + 1e-4 * rng.normal(size=9))
    labels = truth.astype(np.int32)
    labels[truth == 1] = rng.integers(0, 2, size=int((truth == 1).sum()))
    flip = rng.random(n) < 0.15
    labels[flip] = rng.integers(-1, nh, size=int(flip.sum()))
    hits = [list(rng.choice(n, size=3, replace=False)) for _ in range(n)]
    for i in range(0, n, 5):
        hits[int(hits[i][0])].append(i)
    for i in range(0, n, 11):
        hits[i].append(i)
    hits[17] = []
    for i in range(n):
        hits[i] = [q for q in hits[i] if q != 17]
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(h) for h in hits])
    col = np.array([q for h in hits for q in h], dtype=np.int32)
    rp, cl, w = O.build_sym_graph(n, rowptr, col)
    assert {1, 2} <= set(np.unique(w).tolist())
    _cache["case"] = (src, dst, labels, H, rp, cl, w)
    return _cache["case"]


# ---- 1. the contract ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("term", [T.REFERENCE, T.RISING])
def test_the_delta_is_the_energy_change_of_the_drop(term, symmetric):
    src, dst, labels, H, rp, cl, w = _case()
    args = (rp, cl, w, LAM, THR2, term, symmetric)
    before = M.labeling_energy(src, dst, labels, H, *args)
    delta, parts, status, alt = L.drop_deltas(src, dst, labels, H, np.arange(4), *args)
    assert (status == L.OK).all() and (parts[:, 0] == np.bincount(labels[labels >= 0], minlength=4)).all()
    assert (delta == parts[:, 2] - parts[:, 1] + parts[:, 4] - parts[:, 3]).all()
    assert (alt != labels).all() and alt.min() >= -1 and alt.max() <= 3
    moved_to_a_label = 0
    for k in range(4):
        lab2 = L.labels_after_drop(labels, k, alt)
        assert not (lab2 == k).any()
        after = M.labeling_energy(src, dst, lab2, H, *args)
        assert after[0] - before[0] == delta[k], (k, after, before, delta[k])
        assert after[1] - before[1] == parts[k, 2] - parts[k, 1] and after[2] - before[2] == parts[k, 4] - parts[k, 3]
        moved_to_a_label += int((lab2[labels == k] >= 0).sum())
        # ... and in the compacted numbering without model k
        lab3, H3, gone = L.apply_drop(labels, H, k, alt)
        assert M.labeling_energy(src, dst, lab3, H3, *args) == after and gone == int((lab2[labels == k] < 0).sum())
    assert moved_to_a_label > 0                              # (labels 0 and 1 share a plane: their members have somewhere to go)


def test_own_cost_and_alt_cost_are_the_tables_entries():
    src, dst, labels, H, rp, cl, w = _case()
    for term in (T.REFERENCE, T.RISING):
        table = T.cost_table(src, dst, H, LAM, THR2, term).astype(np.int64)
        alt, alt_cost, own_cost = L.best_alternative(src, dst, labels, H, LAM, THR2, term, False)
        rows = np.arange(labels.size)
        assert np.array_equal(own_cost, table[rows, labels + 1]) and np.array_equal(alt_cost, table[rows, alt + 1])
        for i in rows:                                       # no allowed column is cheaper, and no earlier one as cheap
            for l in range(-1, 4):
                if l != labels[i]:
                    assert table[i, l + 1] > alt_cost[i] or (table[i, l + 1] == alt_cost[i] and l >= alt[i])


# ---- 2. the tie rule ----------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_outlier_then_to_the_lowest_index():
    src, dst, labels, H, rp, cl, w = _case()
    n = labels.size
    # equal integer costs by construction: models 1, 2, 3 are one model
    H2 = H.copy()
    H2[2] = H2[3] = H2[1]
    lab = np.zeros(n, dtype=np.int32)
    lab[:8] = [1, 2, 3, 1, 2, 3, -1, -1]
    alt, alt_cost, _ = L.best_alternative(src, dst, lab, H2, LAM, THR2, T.REFERENCE, False)
    rows = L.cost_rows(src, dst, H2, LAM, THR2, T.REFERENCE, False)
    assert np.array_equal(rows[1], rows[2]) and np.array_equal(rows[1], rows[3])
    near = rows[1] < OUTLIER
    on1 = np.flatnonzero((lab == 0) & near & (rows[1] < rows[0]))
    assert on1.size > 10 and (alt[on1] == 1).all()           # 1, 2 and 3 tie: the lowest index
    assert alt[1] in (-1, 0, 1) and alt[0] in (-1, 0, 2)      # a site's own label is no candidate
    # a table with ties against the outlier: the outlier comes first
    table = np.full((n, 5), 7, dtype=np.int64)
    alt, alt_cost, own = L.best_alternative(src, dst, lab, H2, LAM, THR2, T.REFERENCE, False, table=table)
    assert (alt[lab >= 0] == -1).all() and (alt[lab < 0] == 0).all() and (alt_cost == 7).all()
    # every model beyond the threshold: every cost is 2 B against the outlier's B, so the outlier wins for every labelled site,
    # and an outlier's alternative is the lowest used label at 2 B
    far = H.copy()
    far[:, 2] += 1.0e5 * far[:, 8]
    lab = labels.copy()
    alt, alt_cost, own = L.best_alternative(src, dst, lab, far, LAM, THR2, T.RISING, False)
    assert (L.cost_rows(src, dst, far, LAM, THR2, T.RISING, False) == 2 * OUTLIER).all()
    assert (alt[lab >= 0] == -1).all() and (alt_cost[lab >= 0] == OUTLIER).all() and (own[lab >= 0] == 2 * OUTLIER).all()
    assert (alt[lab < 0] == 0).all() and (alt_cost[lab < 0] == 2 * OUTLIER).all() and (own[lab < 0] == OUTLIER).all()
    # dropping a label there sends every member to the outlier label
    delta, parts, status, _ = L.drop_deltas(src, dst, lab, far, [2], rp, cl, w, LAM, THR2, T.RISING, False)
    assert parts[0, 2] - parts[0, 1] == -OUTLIER * parts[0, 0]


def test_unused_labels_are_no_alternative():
    src, dst, labels, H, rp, cl, w = _case()
    lab = np.where(labels == 1, 0, labels).astype(np.int32)  # label 1, the twin model of label 0's plane, is unused
    alt, _, _ = L.best_alternative(src, dst, lab, H, LAM, THR2, T.REFERENCE, False)
    assert not (alt == 1).any()
    alt_all, _, _ = L.best_alternative(src, dst, labels, H, LAM, THR2, T.REFERENCE, False)
    assert (alt_all == 1).any()


# ---- 3. no candidate at all ---------------------------------------------------------------------------------------------------
def test_sites_with_an_empty_candidate_set():
    src, dst, labels, H, rp, cl, w = _case()
    lab = np.full(labels.size, -1, dtype=np.int32)
    alt, alt_cost, own = L.best_alternative(src, dst, lab, H, LAM, THR2, T.REFERENCE, False)
    assert (alt == -1).all() and (alt_cost == OUTLIER).all() and (own == OUTLIER).all()
    delta, parts, status, _ = L.drop_deltas(src, dst, lab, H, [0, 3], rp, cl, w, LAM, THR2, T.REFERENCE, False)
    assert status.tolist() == [L.EMPTY, L.EMPTY] and (delta == L.NO_DELTA).all() and not parts.any()
    # one used label: its members can only become outliers, an outlier can only take it
    lab[:50] = 2
    alt, alt_cost, own = L.best_alternative(src, dst, lab, H, LAM, THR2, T.REFERENCE, False)
    assert (alt[:50] == -1).all() and (alt[50:] == 2).all()
    # no model at all
    alt, alt_cost, own = L.best_alternative(src, dst, np.full(labels.size, -1), np.zeros((0, 9)), LAM, THR2, T.REFERENCE, False)
    assert (alt == -1).all() and (alt_cost == OUTLIER).all()


# ---- 4. a label whose members neighbour only each other -------------------------------------------------------------------------
@pytest.mark.parametrize("term", [T.REFERENCE, T.RISING])
def test_a_label_that_neighbours_only_itself(term):
    src, dst, labels, H, _, _, _ = _case()
    n = labels.size
    lab = labels.copy()
    island = np.arange(40, 70)
    lab[lab == 3] = 2
    lab[island] = 3
    hits = [[] for _ in range(n)]
    rng = np.random.default_rng(5)
    for i in range(n):
        pool = island if i in island else np.setdiff1d(np.arange(n), island)
        hits[i] = [int(q) for q in rng.choice(pool, size=3, replace=False) if q != i]
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(h) for h in hits])
    rp, cl, w = O.build_sym_graph(n, rowptr, np.array([q for h in hits for q in h], dtype=np.int32))
    args = (rp, cl, w, LAM, THR2, term, False)
    delta, parts, status, alt = L.drop_deltas(src, dst, lab, H, [3], *args)
    assert status[0] == L.OK and parts[0, 0] == 30 and parts[0, 3] == 0          # nothing is cut before the drop
    inner = sum(int(w[e]) for p in island for e in range(rp[p], rp[p + 1]) if cl[e] < p and alt[p] != alt[cl[e]])
    assert parts[0, 4] == O.potts(LAM) * inner
    before = M.labeling_energy(src, dst, lab, H, *args)
    after = M.labeling_energy(src, dst, L.labels_after_drop(lab, 3, alt), H, *args)
    assert after[0] - before[0] == delta[0]


# ---- 5. the host's rule and bookkeeping -------------------------------------------------------------------------------------------
def _host_select_merges(host, pairs, delta, status, nh, beta):
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    delta = np.ascontiguousarray(delta, dtype=np.int64)
    status = np.ascontiguousarray(status, dtype=np.int32)
    out = np.full(max(len(delta), 1), -7, dtype=np.int32)
    k = host.mhh_select_merges_label_cost(pairs.ctypes.data_as(_ip), delta.ctypes.data_as(_lp), status.ctypes.data_as(_ip), len(delta), nh,
                                          C.c_longlong(beta), out.ctypes.data_as(_ip))
    return out[:k].tolist()


def _host_select_drop(host, cand, delta, status, beta):
    cand = np.ascontiguousarray(cand, dtype=np.int32)
    delta = np.ascontiguousarray(delta, dtype=np.int64)
    status = np.ascontiguousarray(status, dtype=np.int32)
    return host.mhh_select_drop(cand.ctypes.data_as(_ip), delta.ctypes.data_as(_lp), status.ctypes.data_as(_ip), len(cand), C.c_longlong(beta))


def test_select_merges_with_a_label_cost(host):
    rng = np.random.default_rng(11)
    for trial in range(60):
        nh = int(rng.integers(2, 14))
        allp = np.array([(a, b) for a in range(nh) for b in range(a + 1, nh)], dtype=np.int32)
        pairs = allp[rng.permutation(len(allp))[:int(rng.integers(1, len(allp) + 1))]]
        delta = rng.integers(-6, 9, size=len(pairs)).astype(np.int64)
        status = rng.choice([M.OK, M.OK, M.OK, M.EMPTY, M.NO_FIT], size=len(pairs)).astype(np.int32)
        delta[status != M.OK] = M.NO_DELTA
        if trial % 3 == 0:
            delta[rng.integers(len(pairs))] = -(2 ** 62)
        for beta in (0, 1, 4, 9, 2 ** 62):
            got = _host_select_merges(host, pairs, delta, status, nh, beta)
            assert got == L.select_merges(pairs, delta, status, nh, beta), (trial, beta)
            assert all(status[k] == M.OK and int(delta[k]) - beta < 0 for k in got)
            used = pairs[got].reshape(-1).tolist()
            assert len(used) == len(set(used))
        # beta = 0 is the parent's rule: the twin's, and the host's own SelectMerges
        got0 = _host_select_merges(host, pairs, delta, status, nh, 0)
        assert got0 == M.select_merges(pairs, delta, status, nh)
        out = np.full(len(pairs), -7, dtype=np.int32)
        k = host.mhh_select_merges(pairs.ctypes.data_as(_ip), delta.ctypes.data_as(_lp), status.ctypes.data_as(_ip), len(pairs), nh,
                                   out.ctypes.data_as(_ip))
        assert out[:k].tolist() == got0
    # a delta of exactly beta is not taken; one below is
    assert _host_select_merges(host, [[0, 1], [2, 3]], [5, 4], [0, 0], 4, 5) == [1]


def test_select_drop(host):
    rng = np.random.default_rng(12)
    for trial in range(200):
        nc = int(rng.integers(1, 9))
        cand = rng.permutation(12)[:nc].astype(np.int32)
        delta = rng.integers(-3, 6, size=nc).astype(np.int64)
        status = rng.choice([L.OK, L.OK, L.EMPTY], size=nc).astype(np.int32)
        delta[status != L.OK] = L.NO_DELTA
        for beta in (0, 2, 5, 2 ** 62):
            got = _host_select_drop(host, cand, delta, status, beta)
            assert got == L.select_drop(cand, delta, status, beta), (trial, beta, cand, delta, status)
            if got >= 0:
                assert status[got] == L.OK and int(delta[got]) - beta < 0
    assert _host_select_drop(host, [5, 2, 9], [-4, -4, -1], [0, 0, 0], 0) == 1          # ties on delta: the lower label
    assert _host_select_drop(host, [5, 2], [3, 3], [0, 0], 3) == -1 and _host_select_drop(host, [5, 2], [3, 3], [0, 0], 4) == 1
    assert _host_select_drop(host, [1], [L.NO_DELTA], [L.EMPTY], 2 ** 62) == -1 and _host_select_drop(host, [], [], [], 7) == -1


def test_apply_drop(host):
    rng = np.random.default_rng(13)
    for trial in range(30):
        nh, n = int(rng.integers(1, 9)), 300
        labels = rng.integers(-1, nh, size=n).astype(np.int32)
        H = rng.normal(size=(nh, 9))
        k = int(rng.integers(0, nh))
        alt = rng.integers(-1, nh, size=n).astype(np.int32)
        alt[alt == labels] = -1                               # an alternative is never the own label
        want_lab, want_H, want_gone = L.apply_drop(labels, H, k, alt)
        assert want_H.shape == (nh - 1, 9) and want_lab.max() <= nh - 2
        assert np.array_equal(want_lab[labels != k] == -1, labels[labels != k] == -1)
        lab_h, H_h, gone = labels.copy(), np.ascontiguousarray(H.copy()), C.c_int(-1)
        cnt = host.mhh_apply_drop(k, alt.ctypes.data_as(_ip), n, lab_h.ctypes.data_as(_ip), H_h.ctypes.data_as(_dp), nh, C.byref(gone))
        assert cnt == nh - 1 and np.array_equal(lab_h, want_lab) and R.same_bits(H_h[:cnt], want_H) and gone.value == want_gone


def test_beta_is_stated_in_outliers():
    assert OUTLIER == 4901 and L.beta_of(40, LAM, THR2) == 40 * 4901 and L.beta_of(0.0, LAM, THR2) == 0 and L.beta_of(0.5, LAM, THR2) == 2451


def test_the_margins_of_the_process_scene(mh):
    """The scene of tests/test_gpu_label_cost.py::test_process_drops_the_spurious_label, on the twin: on the truth labeling with
    the patch under its own label, at the cost the issue names (40 outliers' worth) and at the cost that test runs with (1),
    dropping the patch's label pays (delta - beta < 0) and dropping either true plane does not; the margins are printed."""
    sc, init, patch = L.label_cost_scene(mh)
    counts = np.bincount(sc.gt_label[sc.gt_label >= 0])
    assert counts.size == 2 and (counts > 550).all() and (counts < 650).all() and patch.size == 20
    labels = sc.gt_label.astype(np.int32).copy()
    labels[patch] = 2
    init = np.concatenate([sc.H_true / np.linalg.norm(sc.H_true, axis=1, keepdims=True), init[3:4]])      # the truth and the patch's refit
    rp, cl, w = O.build_sym_graph(sc.n, sc.hit_rowptr, sc.hit_col)
    for term in (T.REFERENCE, T.RISING):
        delta, parts, status, alt = L.drop_deltas(sc.src, sc.dst, labels, init, [0, 1, 2], rp, cl, w, LAM, THR2, term, False)
        assert (status == L.OK).all() and parts[2, 0] == 20 and (alt[patch] == 0).all()
        for points in (40, 1):
            beta = L.beta_of(points, LAM, THR2)
            print(term, points, beta, (delta - beta).tolist())
            assert delta[2] - beta < -beta // 2 and delta[0] - beta > 2 * beta and delta[1] - beta > 2 * beta


# ---- 6. exports, weak references, the flag, the resource report -----------------------------------------------------------------
def test_exports_and_weak_references(mh, engine_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", mh.LIB_PATH], capture_output=True, text=True).stdout
    for sym in ("mh_best_alternative", "mh_drop_deltas"):
        assert re.search(r"\bT " + sym + r"\b", out), sym
        assert sym in mh.capi.SYMBOLS
    host = os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so")
    out = subprocess.run(["nm", "-D", host], capture_output=True, text=True).stdout
    # the host class refers to the one call it makes weakly: an engine library without it still loads
    assert re.search(r"\bw mh_drop_deltas\b", out), "mh_drop_deltas must be a weak reference of libmultih_host.so"
    for sym in ("mhh_set_label_cost", "mhh_get_drop_log", "mhh_select_merges_label_cost", "mhh_select_drop", "mhh_apply_drop"):
        assert re.search(r"\bT " + sym + r"\b", out), sym
    assert (mh.capi.DROP_OK, mh.capi.DROP_EMPTY, mh.capi.DROP_NO_DELTA, mh.capi.BEST_ALT_TILE) == (L.OK, L.EMPTY, L.NO_DELTA, L.TILE)


def test_the_harness_takes_the_label_cost_flag(mh, engine_lib, tmp_path):
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    assert os.path.exists(harness), "harness not built"
    r = subprocess.run([harness], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--label-cost P]" in r.stderr
    r = subprocess.run([harness, str(tmp_path / "missing.txt"), str(tmp_path / "out.txt"), "--merge", "energy", "--label-cost", "40"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--label-cost" not in r.stderr and "missing.txt" in r.stderr, (r.returncode, r.stderr)


def test_the_new_kernels_use_no_scratch(mh, tmp_path):
    """All eight instantiations of csrc/label_cost.hip, compiled device-only with the build's flags: no scratch, no spilled
    register, no dynamic stack."""
    import importlib
    b = importlib.import_module("multi-h_amd.build")
    r = subprocess.run([b.HIPCC] + b.HIP_FLAGS + ["--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                  os.path.join(b.CSRC, "label_cost.hip"), "-o", str(tmp_path / "label_cost.s")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"remark: Function Name: (\S+)", r.stderr)
    pretty = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    seen = {"k_best_alternative": 0, "k_drop_label": 0}
    for blk, name in zip(re.split(r"remark: Function Name: ", r.stderr)[1:], pretty):
        m = re.match(r"void mh::(k_best_alternative|k_drop_label)<", name)
        assert m, name
        f = {k.strip(): v.strip() for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+): (\S+) \[-Rpass", blk)}
        print(name.split("(")[0], f.get("VGPRs"), f.get("TotalSGPRs"), f.get("LDS Size [bytes/block]"), f.get("Occupancy [waves/SIMD]"))
        assert f["ScratchSize [bytes/lane]"] == "0" and f["VGPRs Spill"] == "0" and f["SGPRs Spill"] == "0", (name, f)
        assert f["Dynamic Stack"] == "False", (name, f)
        seen[m.group(1)] += 1
    assert seen == {"k_best_alternative": 4, "k_drop_label": 4}
