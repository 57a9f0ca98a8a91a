"""The neighbourhood-guided proposal sampler's numpy twin (tests/local_sampler_numpy.py) against the oracle's uniform sampler
and against the properties the rule promises.  No GPU: the engine's tuples are compared with this twin in
tests/test_gpu_local_sampler.py."""
import numpy as np
import pytest

import local_sampler_numpy as twin

SEED = 99


@pytest.fixture(scope="module")
def scene(mh):
    sc = mh.synth.make_scene(2000, 5, seed=7, with_neighbours=False)
    return sc, twin.knn_table(sc.src, sc.dst, 8)


@pytest.mark.parametrize("first", [0, 10, (1 << 40) + 5])
def test_sixteen_uniform_per_sixteen_is_the_uniform_sampler(oracle, scene, first):
    sc, nbr = scene
    want = oracle.sample4(SEED, first, 500, sc.src.shape[0])
    assert np.array_equal(twin.sample_local(SEED, first, 500, sc.src.shape[0], nbr, 16), want)
    assert np.array_equal(twin.sample_uniform(SEED, first, 500, sc.src.shape[0]), want)


def test_the_twin_wraps_like_the_oracle_where_seed_plus_counter_overflows(oracle):
    # seed + (c << 8) passes 2^64 inside the batch: c << 8 = 2^64 - 512 .. and the seed adds 1000
    n, first, seed = 300, (1 << 56) - 2, 1000
    assert np.array_equal(twin.sample_uniform(seed, first, 40, n), oracle.sample4(seed, first, 40, n))


@pytest.mark.parametrize("u", [0, 4, 8])
def test_first_index_uniform_positions_and_membership(oracle, scene, u):
    sc, nbr = scene
    n, first, m = sc.src.shape[0], 10, 1000
    uni = oracle.sample4(SEED, first, m, n)
    loc = twin.sample_local(SEED, first, m, n, nbr, u)
    assert np.array_equal(loc[:, 0], uni[:, 0]), "a local tuple starts where the uniform tuple starts"
    c = first + np.arange(m)
    is_uniform = (c & 15) < u
    assert np.array_equal(loc[is_uniform], uni[is_uniform]), "the uniform share of a mixed batch is the uniform batch there"
    for t in loc[~is_uniform]:
        assert set(t[1:].tolist()) <= set(nbr[t[0]].tolist()) | {int(t[0])}, "indices after the first come from nbr[i0]"
        assert len(set(t.tolist())) == 4                  # k = 8 >= 3 distinct neighbours: 63 draws do not run out here


def test_exhaustion_takes_the_first_index():
    # a table whose rows offer one candidate only: slots 2 and 3 stay empty after draw 63 and take out[0]
    n = 50
    nbr = np.tile(((np.arange(n) + 1) % n)[:, None], (1, 3)).astype(np.int32)
    loc = twin.sample_local(SEED, 0, 64, n, nbr, 0)
    assert np.array_equal(loc[:, 1], (loc[:, 0] + 1) % n)
    assert np.array_equal(loc[:, 2], loc[:, 0]) and np.array_equal(loc[:, 3], loc[:, 0])


def test_same_plane_share(scene):
    """The point of the sampler: on 2000 points / 5 planes (k = 8, 4000 tuples) well over half of the local tuples lie on one
    true plane, of the uniform ones next to none (about sum_k share_k^4).  Measured with this twin: 0.7455 and 0.004."""
    sc, nbr = scene
    n = sc.src.shape[0]
    loc = twin.same_plane_share(twin.sample_local(SEED, 0, 4000, n, nbr, 0), sc.gt_label)
    uni = twin.same_plane_share(twin.sample_uniform(SEED, 0, 4000, n), sc.gt_label)
    print(f"same-plane share: local {loc:.4f}, uniform {uni:.4f}")
    assert loc >= 0.5
    assert uni <= 0.02


def test_table_rule_on_ties_and_duplicates():
    # integer coordinates: exact float32 distances, ties at rank k decided by the lower index, a duplicate point at distance 0
    src = np.array([[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1], [0, 0], [5, 5]], dtype=np.float64)
    dst = np.zeros_like(src)
    nbr = twin.knn_table(src, dst, 3)
    assert nbr[0].tolist() == [5, 1, 2]                       # the duplicate first, then the four at distance 1 by index
    assert nbr[5].tolist() == [0, 1, 2]
    assert nbr[6].tolist() == [1, 2, 0]                       # d = 41, 41, 50 (0 and 5 tie at 50: the lower index)
