"""The energy-tested merge without a GPU: the twin's contract (tests/merge_energy_numpy.py: the energy after relabelling b -> a with
H_ab as model a, minus the energy before, is pair_delta's delta — under both data terms and both errors, and the deltas of pairs
that share no label add), the host's SelectMerges against the twin's rule on random tables (host/merge_step.cpp through
mhh_select_merges), and the bookkeeping of apply_merges / ApplyMerges."""
import ctypes as C
import os

import numpy as np
import pytest

import data_term_numpy as T
import merge_energy_numpy as M
import oracle_lib as O
import refit_h_numpy as R

LAM, THR2 = 0.5, 2.2 ** 2
_cache = {}


@pytest.fixture(scope="module")
def host(mh, engine_lib):
    lib = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    assert hasattr(lib, "mhh_select_merges") and hasattr(lib, "mhh_apply_merges")
    return lib


def _case():
    """360 points on four noisy planes with near-true models, a labeling with outliers and wrong labels, and directed hit lists
    with one-way hits (w = 1), mutual hits (w = 2), self hits and an isolated site.  Computed once."""
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
    H[1] = H[0] * (1.0 + 1e-4 * rng.normal(size=9))          # two models of nearly one plane: data terms inside the threshold
    labels = truth.astype(np.int32)
    labels[truth == 1] = rng.integers(0, 2, size=int((truth == 1).sum()))
    flip = rng.random(n) < 0.15
    labels[flip] = rng.integers(-1, nh, size=int(flip.sum()))
    hits = [list(rng.choice(n, size=3, replace=False)) for _ in range(n)]
    for i in range(0, n, 5):
        hits[int(hits[i][0])].append(i)                      # a mutual hit
    for i in range(0, n, 11):
        hits[i].append(i)                                    # a self hit
    hits[17] = []
    for i in range(n):
        hits[i] = [q for q in hits[i] if q != 17]            # site 17: isolated
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(h) for h in hits])
    col = np.array([q for h in hits for q in h], dtype=np.int32)
    rp, cl, w = O.build_sym_graph(n, rowptr, col)
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert {1, 2} <= set(np.unique(w).tolist()) and not (rows == cl).any() and rp[18] == rp[17]     # (a self hit makes no arc)
    _cache["case"] = (src, dst, labels, H, rp, cl, w)
    return _cache["case"]


PAIRS = [(a, b) for a in range(4) for b in range(a + 1, 4)]


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("term", [T.REFERENCE, T.RISING])
def test_the_delta_is_the_energy_change_of_the_relabel(term, symmetric):
    src, dst, labels, H, rp, cl, w = _case()
    args = (rp, cl, w, LAM, THR2, term, symmetric)
    before = M.labeling_energy(src, dst, labels, H, *args)
    assert before[0] == before[1] + before[2]
    Hs, delta, parts, status = M.merge_deltas(src, dst, labels, H, PAIRS, *args)
    assert (status == M.OK).all()
    assert (parts[:, 0] == [(np.isin(labels, p)).sum() for p in PAIRS]).all()
    assert (delta == parts[:, 2] - parts[:, 1] - parts[:, 3]).all() and (parts[:, 3] > 0).all()
    for k in range(len(PAIRS)):
        lab2, H2 = M.apply_merges(labels, H, PAIRS, Hs, [k])
        after = M.labeling_energy(src, dst, lab2, H2, *args)
        assert after[0] - before[0] == delta[k], (PAIRS[k], after, before, delta[k])
        assert after[2] - before[2] == -parts[k, 3]
    # two pairs that share no label: the deltas add
    both = [PAIRS.index((0, 1)), PAIRS.index((2, 3))]
    lab2, H2 = M.apply_merges(labels, H, PAIRS, Hs, both)
    assert H2.shape == (2, 9) and set(np.unique(lab2).tolist()) == {-1, 0, 1}
    assert M.labeling_energy(src, dst, lab2, H2, *args)[0] - before[0] == delta[both].sum()


def test_labels_of_nobody_and_the_statuses():
    src, dst, labels, H, rp, cl, w = _case()
    args = (rp, cl, w, LAM, THR2, T.REFERENCE, False)
    want = M.pair_delta(src, dst, labels, H, 0, 1, *args)
    foreign = labels.copy()
    out = np.flatnonzero(labels == -1)
    foreign[out[::2]] = 4                                    # Nh
    foreign[out[1::2]] = 1 << 20
    got = M.pair_delta(src, dst, foreign, H, 0, 1, *args)
    assert got[0] == M.OK and got[2:] == want[2:] and R.same_bits(got[1], want[1])
    # an empty side; 1 + 2 members; 2 + 2 members
    lab = np.full(labels.size, -1, dtype=np.int32)
    lab[:3] = 0
    assert M.pair_delta(src, dst, lab, H, 0, 1, *args)[0::3] == (M.EMPTY, M.NO_DELTA)
    lab[2] = 1
    assert M.pair_delta(src, dst, lab, H, 0, 1, *args)[0::3] == (M.NO_FIT, M.NO_DELTA)
    lab[3] = 1
    st, h, parts, delta = M.pair_delta(src, dst, lab, H, 0, 1, *args)
    assert st == M.OK and parts[0] == 4 and R.same_bits(h, R.fit(src, dst, np.arange(4)))


def _host_select(host, pairs, delta, status, nh):
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    delta = np.ascontiguousarray(delta, dtype=np.int64)
    status = np.ascontiguousarray(status, dtype=np.int32)
    out = np.full(max(len(delta), 1), -7, dtype=np.int32)
    k = host.mhh_select_merges(pairs.ctypes.data_as(C.POINTER(C.c_int)), delta.ctypes.data_as(C.POINTER(C.c_longlong)),
                               status.ctypes.data_as(C.POINTER(C.c_int)), len(delta), nh, out.ctypes.data_as(C.POINTER(C.c_int)))
    return out[:k].tolist()


def test_select_merges_is_the_twins_rule(host):
    rng = np.random.default_rng(11)
    for trial in range(60):
        nh = int(rng.integers(2, 14))
        allp = np.array([(a, b) for a in range(nh) for b in range(a + 1, nh)], dtype=np.int32)
        pairs = allp[rng.permutation(len(allp))[:int(rng.integers(1, len(allp) + 1))]]
        delta = rng.integers(-6, 4, size=len(pairs)).astype(np.int64)      # few values: ties, zeros
        status = rng.choice([M.OK, M.OK, M.OK, M.EMPTY, M.NO_FIT], size=len(pairs)).astype(np.int32)
        delta[status != M.OK] = M.NO_DELTA
        if trial % 3 == 0:
            delta[rng.integers(len(pairs))] = -(2 ** 62)
        got = _host_select(host, pairs, delta, status, nh)
        assert got == M.select_merges(pairs, delta, status, nh), (trial, pairs.tolist(), delta.tolist(), status.tolist())
        used = pairs[got].reshape(-1).tolist()
        assert len(used) == len(set(used)), "a label was used twice"
        assert all(delta[k] < 0 and status[k] == M.OK for k in got)
        # nothing acceptable is left behind: every other OK pair with a negative delta shares a label with an accepted one
        for k in range(len(pairs)):
            if k not in got and status[k] == M.OK and delta[k] < 0:
                assert set(pairs[k].tolist()) & set(used)
    assert _host_select(host, np.zeros((0, 2), np.int32), np.zeros(0, np.int64), np.zeros(0, np.int32), 5) == []
    # ties on delta go by (a, b)
    assert _host_select(host, [[2, 3], [0, 1], [0, 2]], [-5, -5, -5], [0, 0, 0], 4) == [1, 0]


def test_apply_merges_keeps_the_partition_and_renumbers_densely(host):
    rng = np.random.default_rng(12)
    for trial in range(20):
        nh, n = int(rng.integers(2, 12)), 300
        labels = rng.integers(-1, nh, size=n).astype(np.int32)
        H = rng.normal(size=(nh, 9))
        perm = rng.permutation(nh)
        pairs = np.sort(perm[:2 * (nh // 2)].reshape(-1, 2), axis=1).astype(np.int32)      # disjoint pairs
        accepted = [k for k in range(len(pairs)) if rng.random() < 0.6]
        H_ab = rng.normal(size=(len(pairs), 9))
        lab2, H2 = M.apply_merges(labels, H, pairs, H_ab, accepted)
        assert H2.shape[0] == nh - len(accepted)
        assert np.array_equal(lab2 == -1, labels == -1)
        assert set(np.unique(lab2[lab2 >= 0]).tolist()) <= set(range(H2.shape[0]))
        # two points share a label afterwards iff they did before or their labels were joined
        joined = np.arange(nh)
        for k in accepted:
            joined[pairs[k, 1]] = pairs[k, 0]
        cls = np.where(labels >= 0, joined[np.maximum(labels, 0)], -1)
        assert np.array_equal(cls[:, None] == cls[None, :], lab2[:, None] == lab2[None, :])
        # the models: a joined pair's a carries H_ab, the others their own, in the old order
        survivors = [l for l in range(nh) if l not in set(pairs[accepted, 1].tolist())]
        for new, old in enumerate(survivors):
            hit = [k for k in accepted if pairs[k, 0] == old]
            assert R.same_bits(H2[new], H_ab[hit[0]] if hit else H[old])
            assert (lab2[cls == old] == new).all()
        # the host's ApplyMerges does the same
        lab_h, H_h = labels.copy(), np.ascontiguousarray(H.copy())
        acc = np.ascontiguousarray(accepted, dtype=np.int32)
        cnt = host.mhh_apply_merges(pairs.ctypes.data_as(C.POINTER(C.c_int)), np.ascontiguousarray(H_ab).ctypes.data_as(C.POINTER(C.c_double)),
                                    acc.ctypes.data_as(C.POINTER(C.c_int)), len(accepted), n, lab_h.ctypes.data_as(C.POINTER(C.c_int)),
                                    H_h.ctypes.data_as(C.POINTER(C.c_double)), nh)
        assert cnt == H2.shape[0] and np.array_equal(lab_h, lab2) and R.same_bits(H_h[:cnt], H2)


def test_the_harness_takes_the_merge_flag(mh, engine_lib, tmp_path):
    import subprocess
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    assert os.path.exists(harness), "harness not built"
    r = subprocess.run([harness, str(tmp_path / "in.txt"), str(tmp_path / "out.txt"), "--merge", "bogus"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "--merge: meanshift or energy" in r.stderr
    r = subprocess.run([harness], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--merge meanshift|energy]" in r.stderr
    # the value itself is taken: the run gets as far as the input file, which is not there (no GPU is touched before that)
    for word in ("meanshift", "energy"):
        r = subprocess.run([harness, str(tmp_path / "missing.txt"), str(tmp_path / "out.txt"), "--merge", word],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--merge" not in r.stderr and "missing.txt" in r.stderr, (r.returncode, r.stderr)


def _pair_list(host, H, all_up_to, nearest):
    H = np.ascontiguousarray(H, dtype=np.float64)
    nh = H.shape[0]
    out = np.full((nh * max(nh - 1, nearest, 1), 2), -7, dtype=np.int32)
    k = host.mhh_merge_pair_list(H.ctypes.data_as(C.POINTER(C.c_double)), nh, all_up_to, nearest, out.ctypes.data_as(C.POINTER(C.c_int)))
    return out[:k]


def _features(H):
    """The 6-D merge feature: the images of (0, 0), (1, 0), (0, 1) (what the host computes in HomographyFeatures)."""
    h = np.asarray(H, np.float64)
    with np.errstate(all="ignore"):
        return np.stack([h[:, 2] / h[:, 8], h[:, 5] / h[:, 8], (h[:, 0] + h[:, 2]) / (h[:, 6] + h[:, 8]),
                         (h[:, 3] + h[:, 5]) / (h[:, 6] + h[:, 8]), (h[:, 1] + h[:, 2]) / (h[:, 7] + h[:, 8]),
                         (h[:, 4] + h[:, 5]) / (h[:, 7] + h[:, 8])], axis=1)


def test_the_pair_list(host):
    """MergePairList: all pairs up to the bound; beyond it every label's `nearest` nearest labels in the feature space, as a < b,
    sorted, without duplicates; a label whose features are not finite is nobody's neighbour and has none."""
    rng = np.random.default_rng(13)
    for nh in (1, 2, 5, 9):
        H = rng.normal(size=(nh, 9))
        want = [(a, b) for a in range(nh) for b in range(a + 1, nh)]
        assert [tuple(p) for p in _pair_list(host, H, 64, 8).tolist()] == want
        assert [tuple(p) for p in _pair_list(host, H, nh, 8).tolist()] == want      # nh == all_up_to: still all pairs
    for nh, nearest in ((12, 3), (40, 8), (6, 8), (30, 1)):
        H = np.eye(3).reshape(9) + 0.05 * rng.normal(size=(nh, 9))
        H[:, 2] += rng.uniform(-50, 50, size=nh)
        H[:, 5] += rng.uniform(-50, 50, size=nh)
        broken = nh > 10
        if broken:
            H[4, 8] = 0.0                                    # features of label 4: infinite / NaN
        got = [tuple(p) for p in _pair_list(host, H, 4, nearest).tolist()]
        feat = _features(H)
        with np.errstate(all="ignore"):
            d = ((feat[:, None, :] - feat[None, :, :]) ** 2).sum(-1)
        d[~np.isfinite(d)] = np.inf
        np.fill_diagonal(d, np.inf)
        take = min(nearest, nh - 1)
        want = set()
        for a in range(nh):
            order = sorted(range(nh), key=lambda b: (d[a, b], b))[:take]
            want |= {(min(a, b), max(a, b)) for b in order if np.isfinite(d[a, b])}
        assert got == sorted(set(got)) and all(0 <= a < b < nh for a, b in got)
        finite = {p for p in got if not (broken and 4 in p)}
        assert finite == {p for p in want if not (broken and 4 in p)}, (nh, nearest)
        # every label with finite features meets its `take` nearest ones
        for a in range(nh):
            if not (broken and a == 4):
                assert sum(1 for p in got if a in p) >= min(take, nh - 1 - (1 if broken else 0))


def test_select_merges_skips_what_is_not_a_pair(host):
    """The host rule does not trust its table: a row with a >= b or a label outside [0, nh) is passed over, whatever its delta."""
    pairs = [[1, 1], [2, 1], [-1, 2], [0, 5], [3, 4], [0, 2]]
    delta = [-100, -90, -80, -70, -60, -50]
    assert _host_select(host, pairs, delta, [0] * 6, 5) == [4, 5]
    assert _host_select(host, pairs, delta, [0] * 6, 4) == [5]
