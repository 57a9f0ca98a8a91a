"""The HAF proposer's numpy twin (tests/haf_propose_numpy.py) against the oracle, and what the built libraries must offer.
No GPU: the engine's batches are compared with this twin in tests/test_gpu_haf_propose.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import haf_propose_numpy as twin

THR2 = 6.25


@pytest.fixture(scope="module")
def scene(mh):
    sc = mh.synth.make_scene(600, 3, seed=99, with_neighbours=False)
    return sc, twin.knn_table(sc.src, sc.dst, 32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_members_zero_is_the_oracles_haf_point(oracle, scene):
    sc, _ = scene
    want, _ = oracle.haf_point(sc.src, sc.dst, sc.aff, sc.F, sc.e2, 0.0)
    H, used = twin.propose(sc.src, sc.dst, sc.aff, sc.F, sc.e2, 0, sc.n, 1, 0, THR2)
    assert np.isfinite(want).all()
    assert np.array_equal(_bits(H), _bits(want)) and not used.any()
    # ... and the twin's own arithmetic (rows, ten sums, solve) gives those bits too: 600 of 600 rows
    terms = twin.haf_terms(twin.haf_rows(sc.src, sc.dst, sc.aff, sc.F, sc.e2))
    own = np.array([twin.solve(terms[i], sc.F, sc.e2) for i in range(sc.n)])
    same = (_bits(own) == _bits(want)).all(axis=1)
    print(f"rows of the twin's own solve equal to mho_haf_point: {int(same.sum())} of {sc.n}")
    assert same.all()


def test_refits_agree_with_the_oracles_nonminimal_estimator(oracle, scene):
    """The same member sets through mho_haf_reestimate (strided-tree sums, the 1 / lambda rescale): equal after the h33
    normalisation to the project's bound for homographies, 1e-6 relative (measured: 3.5e-11 at the worst of 120 anchors)."""
    sc, nbr = scene
    H, used = twin.propose(sc.src, sc.dst, sc.aff, sc.F, sc.e2, 0, 120, 5, 16, THR2, nbr)
    worst, refitted = 0.0, 0
    for s, i in enumerate(twin.anchors(0, 120, 5)):
        if not used[s] or not np.isfinite(H[s]).all():
            continue
        labels = np.full(sc.n, -1, dtype=np.int32)
        labels[i] = 0
        labels[nbr[i, :16][(used[s] >> np.arange(16, dtype=np.uint32)) & 1 == 1]] = 0
        ref, cnt = oracle.haf_reestimate(sc.src, sc.dst, sc.aff, labels, np.zeros((1, 9)), sc.F, sc.e2)
        assert cnt[0] == 1 + bin(int(used[s])).count("1")
        ref = ref[0] * (1.0 / ref[0, 8])
        worst = max(worst, float(np.max(np.abs(H[s] - ref)) / np.max(np.abs(ref))))
        refitted += 1
    print(f"{refitted} refitted anchors of 120, worst relative difference {worst:.3e}")
    assert refitted >= 60
    assert worst <= 1e-6


@pytest.mark.parametrize("members", [3, 16, 32])
def test_zero_threshold_gives_the_single_correspondence_batch(scene, members):
    sc, nbr = scene
    H0, _ = twin.propose(sc.src, sc.dst, sc.aff, sc.F, sc.e2, 0, sc.n, 1, 0, 0.0)
    H, used = twin.propose(sc.src, sc.dst, sc.aff, sc.F, sc.e2, 0, sc.n, 1, members, 0.0, nbr)
    assert not used.any() and np.array_equal(_bits(H), _bits(H0))


def test_counters_strides_and_shards(scene):
    sc, nbr = scene
    assert twin.anchors(3, 4, 7).tolist() == [21, 28, 35, 42]
    whole, used = twin.propose(sc.src, sc.dst, sc.aff, sc.F, sc.e2, 0, sc.n, 1, 16, THR2, nbr)
    m7 = (sc.n + 6) // 7
    assert m7 == 86
    strided, used7 = twin.propose(sc.src, sc.dst, sc.aff, sc.F, sc.e2, 0, m7, 7, 16, THR2, nbr)
    assert np.array_equal(_bits(strided), _bits(whole[::7])) and np.array_equal(used7, used[::7])
    shard, used_s = twin.propose(sc.src, sc.dst, sc.aff, sc.F, sc.e2, 40, 46, 7, 16, THR2, nbr)
    assert np.array_equal(_bits(shard), _bits(strided[40:])) and np.array_equal(used_s, used7[40:])
    empty, used_e = twin.propose(sc.src, sc.dst, sc.aff, sc.F, sc.e2, 5, 0, 7, 16, THR2, nbr)
    assert empty.shape == (0, 9) and used_e.shape == (0,)
    # members is a prefix of the row: the mask over 3 members is the low three bits of the mask over 16
    _, used3 = twin.propose(sc.src, sc.dst, sc.aff, sc.F, sc.e2, 0, sc.n, 1, 3, THR2, nbr)
    assert np.array_equal(used3, used & np.uint32(7))


def _one_plane(mh, n):
    return mh.synth.make_scene(n, 1, seed=5, with_neighbours=False)


def test_the_twin_leaves_out_at_most_one_row_in_a_hundred(mh, scene):
    """The GPU tests compare bit for bit on every row the twin leaves finite; on their scenes that must be (nearly) all."""
    sc, nbr = scene
    cases = [(sc, nbr, mem, thr2) for mem in (3, 16, 32) for thr2 in (THR2, np.inf)]
    for n in (5, 33, 63, 64, 65):
        one = _one_plane(mh, n)
        k = min(32, n - 1)
        tbl = twin.knn_table(one.src, one.dst, k)
        cases += [(one, tbl, mem, thr2) for mem in (3, 16, 32) if mem <= k for thr2 in (THR2, np.inf)]
    for s, tbl, mem, thr2 in cases:
        H, _ = twin.propose(s.src, s.dst, s.aff, s.F, s.e2, 0, s.n, 1, mem, thr2, tbl)
        left_out = int((~np.isfinite(H).all(axis=1)).sum())
        print(f"n = {s.n}, members = {mem}, thr2 = {thr2}: {left_out} rows not finite")
        assert left_out <= 0.01 * s.n


def test_the_library_exports_the_entry_points(mh, engine_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", mh.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (mh_\w+)", out))
    assert {"mh_propose_haf", "mh_get_haf_support"} <= exported
    assert {"mh_propose_haf", "mh_get_haf_support"} <= set(mh.SYMBOLS)
    host = os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so")
    out = subprocess.run(["nm", "-D", "--defined-only", host], capture_output=True, text=True).stdout
    assert "mhh_set_proposal_source" in out


def test_the_harness_refuses_an_unknown_proposal_source(mh, engine_lib, tmp_path):
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    assert os.path.exists(harness), "harness not built"
    for bad in ("bogus", "haf:2", "haf:16:0", "haf:x"):
        r = subprocess.run([harness, str(tmp_path / "in.txt"), str(tmp_path / "out.txt"), "--proposals", bad],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
        assert "--proposals" in r.stderr and "dlt" in r.stderr and "haf" in r.stderr
