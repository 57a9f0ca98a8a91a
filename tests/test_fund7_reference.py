"""CPU tests of the yardstick the 7-point estimator is measured with (tests/fund7_numpy.py): the twin's two routes to the
solution set agree, and the stop-rule replay gives the values worked out by hand.  No engine involved."""
import math

import numpy as np
import pytest

import fund7_numpy as T


@pytest.mark.parametrize("n", [7, 8, 64])
def test_two_routes_give_the_same_solution_sets(n):
    src, dst = T.make_scene(n, seed=101 + n, noise=0.5)
    rng = np.random.default_rng(n)
    worst_match = worst_res = 0.0
    skipped = 0
    tuples = 300
    for _ in range(tuples):
        idx = rng.permutation(n)[:7]
        Fa, gap = T.solve7(src[idx], dst[idx], route=0)
        Fb, _ = T.solve7(src[idx], dst[idx], route=1)
        if gap < 1e-3:
            skipped += 1
            continue
        assert len(Fa) == len(Fb) and len(Fa) in (1, 3)
        worst_match = max(worst_match, T.set_distance(Fa, Fb), T.set_distance(Fb, Fa))
        for F in Fa:
            det, res = T.constraint_residuals(F, src[idx], dst[idx])
            assert abs(np.linalg.norm(F) - 1.0) <= 1e-12 and F[8] >= 0.0
            worst_res = max(worst_res, det, float(res.max()))
    print(f"n={n}: worst set distance {worst_match:.3g}, worst residual {worst_res:.3g}, skipped {skipped}/{tuples}")
    assert worst_match <= 1e-6
    assert worst_res <= 1e-9
    assert skipped <= tuples // 100


def test_stop_rule_replay_by_hand():
    n, c = 64, 0.99
    S = 50
    # best = n in the first sample: one sample is enough
    counts = np.zeros((S, 3), dtype=np.int32)
    counts[0, 1] = n
    assert T.ransac_stop_replay(counts, n, c)[:3] == (1, 1, n)
    # nothing ever scores: all S samples are used, the winner is slot 0 with count 0
    assert T.ransac_stop_replay(np.zeros((S, 3), dtype=np.int32), n, c)[:3] == (S, 0, 0)
    # in between.  best = 32 of 64 from sample 2 on: w^7 = 2^-7, N = ceil(ln 0.01 / ln(1 - 2^-7)) = ceil(587.2) -> clamped to 50;
    # best = 56 of 64 from sample 4 (slot 2) on: w^7 = 0.875^7 = 0.39270, N = ceil(-4.60517 / -0.49873) = ceil(9.234) = 10,
    # so the run ends after sample index 9: samples_used = 10.  A later, larger count (sample 20) is never seen, and an equal
    # count at a higher index (sample 6) does not take the win.
    counts = np.zeros((S, 3), dtype=np.int32)
    counts[2, 0] = 32
    counts[4, 2] = 56
    counts[6, 0] = 56
    counts[20, 0] = 64
    assert math.ceil(math.log(0.01) / math.log(1.0 - 0.875 ** 7)) == 10
    used, win, best, margin = T.ransac_stop_replay(counts, n, c)
    assert (used, win, best) == (10, 3 * 4 + 2, 56)
    assert margin > 1e-3
    # S = 1 is a run of one sample whatever it scores
    assert T.ransac_stop_replay(np.array([[0, 9, 9]]), n, c)[:3] == (1, 1, 9)
