"""CPU tests of the per-label fits and the moment sums: the oracle against the plain definitions of tests/per_label_numpy.py.

The GPU suite holds k_haf_reestimate and k_moments to the oracle bit for bit, and the oracle sums in the kernels' own order
(256 strided lanes, then a binary tree).  A mistake both share in how the members are visited would pass there.  Here the
oracle is compared with the definition itself (the 6 m x 4 design matrix, A^T A in extended precision, eigh; exactly rounded
moment sums, eigvalsh) on the label patterns of per_label_numpy.edge_labels, at sizes on both sides of 256 and of the
8192 points k_haf_reestimate reads per trip.  Nothing here needs a GPU."""
import functools
import math

import numpy as np
import pytest

import per_label_numpy as P

THR2 = 2.2 * 2.2
EPS = 2.0 ** -52
NH = 12                                    # 3 planes + the nine patterns a .. i
SEEDS = {257: 41, 8193: 42, 16641: 43}     # chosen so that no checked label's bound exceeds GAP_LIMIT (asserted below)
GAP_LIMIT = 1e-6
HAF_MARGIN = 8.6e-4                       # see test_haf_fit_of_the_oracle_is_the_definitions
MIN_EIG_FACTOR = 16.0                      # see test_moments_of_the_oracle_are_the_exact_sums


@functools.lru_cache(maxsize=None)
def _case(synth, oracle, n):
    sc = synth.make_scene(n, 3, seed=SEEDS[n], with_neighbours=False)
    rng = np.random.default_rng(SEEDS[n])
    labels, where = P.edge_labels(n, NH, rng, sc.gt_label)
    H0 = np.tile(sc.H_true, (NH // 3, 1)) * (1.0 + rng.normal(0, 1e-3, (NH, 9)))
    H, cnt = oracle.haf_reestimate(sc.src, sc.dst, sc.aff, labels, H0, sc.F, sc.e2)
    for a in (labels, H0, H, cnt):
        a.setflags(write=False)
    return sc, labels, where, H0, H, cnt


def _scaled(h):
    return h / h[np.argmax(np.abs(h))]


@pytest.mark.parametrize("n", sorted(SEEDS))
def test_counts_and_empty_labels(synth, oracle, n):
    sc, labels, where, H0, H, cnt = _case(synth, oracle, n)
    assert set("abcdi") <= set(where) and len(where["stray"]) == 4
    if n > 8192:
        assert set("efh") <= set(where)
        assert cnt[where["h"]] == 256 if n >= 41 * 256 else 240 <= cnt[where["h"]] < 256
    if n > 8193:
        assert "g" in where and P.members_of(labels, where["g"]).min() >= 8192
    assert np.array_equal(cnt, P.in_range_counts(labels, NH))
    assert [int(cnt[where[p]]) for p in "abcdi"] == [0, 1, 2, 3, 3]
    empty = np.flatnonzero(cnt == 0)
    assert where["a"] in empty
    assert np.array_equal(H[empty].view(np.uint64), H0[empty].view(np.uint64)), "a label without members keeps its H"
    assert not np.array_equal(H[0], H0[0])


@pytest.mark.parametrize("n", sorted(SEEDS))
def test_haf_fit_of_the_oracle_is_the_definitions(synth, oracle, n):
    """oracle.haf_reestimate against per_label_numpy.haf_fit, both scaled by their entry of largest magnitude, for every
    label but the empty ones and patterns (b), (c), (d).

    The allowed distance is HAF_MARGIN * |E| / gap: an eigenvector moves by at most |E| / gap, gap = lambda_2 - lambda_1 of
    the definition's A^T A, and |E| <= (ceil(n_l / 256) + 10) * 2^-52 * |A^T A|_F bounds the rounding of the tree sum.  The
    margin over it stands for the rounding of the 4 x 4 Jacobi and of the assembly of H.  It was measured once, on the CPU, as
    the largest distance / bound of the ORACLE against the definition over the checked labels of the three cases of this file
    (n = 257 / 8193 / 16 641, make_scene(n, 3, seed = 41 / 42 / 43, legacy planes), edge_labels with Nh = 12):
        worst ratio 2.13e-4 (n = 257, plane 2, 17 members: distance 4.4e-13, bound 2.1e-9); per size 2.1e-4 / 1.4e-5 / 8.2e-6
        HAF_MARGIN = 8.6e-4, a factor of 4 over it
    (the bound is that loose because the rounding is nowhere near the worst perturbation of |E|'s size: the smallest
    eigenvector lies almost wholly along the fourth column, whose entries are those of F, ten orders below the others).

    Labels with 1, 2 or 3 members drawn from one plane have no usable gap (lambda_2 is then 1e1 .. 1e4 against |A^T A|_F of
    1e13, the bound 1e-6 .. 1e-3): they are compared for their finiteness pattern only, and they are the only ones skipped.
    Pattern (i) has 3 members as well, but spread over the image, and is checked."""
    sc, labels, where, H0, H, cnt = _case(synth, oracle, n)
    skipped, checked, worst = [], 0, 0.0
    for l in range(NH):
        m = P.members_of(labels, l)
        if m.size == 0:
            continue
        H_def, w, norm = P.haf_fit(sc.src, sc.dst, sc.aff, m, sc.F, sc.e2)
        assert np.array_equal(np.isfinite(H[l]), np.isfinite(H_def)), l
        if m.size < 4 and l != where["i"]:
            skipped.append(l)
            continue
        gap = w[1] - w[0]
        bound = (math.ceil(m.size / 256) + 10) * EPS * norm / gap
        assert bound <= GAP_LIMIT, f"label {l} ({m.size} members): bound {bound:.3g}, choose another seed"
        dist = float(np.linalg.norm(_scaled(H[l]) - _scaled(H_def)))
        print(f"n={n} label {l}: {m.size} members, bound {bound:.3g}, distance {dist:.3g}, ratio {dist / bound:.3g}")
        worst = max(worst, dist / bound)
        assert dist <= HAF_MARGIN * bound, (l, m.size, dist, bound)
        checked += 1
    print(f"n={n}: worst distance / bound {worst:.3g}")
    assert sorted(skipped) == sorted(where[p] for p in "bcd")
    assert checked == NH - 3 - np.count_nonzero(cnt == 0) and checked >= 4


@pytest.mark.parametrize("n", sorted(SEEDS))
def test_moments_of_the_oracle_are_the_exact_sums(synth, oracle, n):
    """oracle.inlier_moments against per_label_numpy.moments: the counts are equal; each of the five sums lies within
    (ceil(n / 256) + 9) * 2^-52 * sum|term| of the exactly rounded sum (a lane adds at most ceil(n / 256) terms, the tree
    eight levels more, one rounding is fsum's: derived, not measured); min_eig lies within
    MIN_EIG_FACTOR * 2^-52 * |M|_F of eigvalsh of the exact sums' matrix.  Measured once, on the CPU, on the models below
    over the three cases of this file: the largest |min_eig - eigvalsh| / (2^-52 |M|_F) was 0.0334 (n = 257; per size
    0.0334 / 7.1e-4 / 9.4e-6): |M|_F is Sxx + Syy, 1e7 .. 1e10, while the error follows the small eigenvalue itself.  The
    factor 16 the check allows is far above four times that."""
    sc, *_ = _case(synth, oracle, n)
    rng = np.random.default_rng(n)
    far = np.array([1, 0, 1e5, 0, 1, 1e5, 0, 0, 1.0])                       # no inliers
    only_last = np.array([0, 0, sc.dst[-1, 0], 0, 0, sc.dst[-1, 1], 0, 0, 1.0])   # maps everything onto dst[n - 1]
    H = np.concatenate([sc.H_true, sc.H_true * (1.0 + rng.normal(0, 2e-4, sc.H_true.shape)),
                        [far, np.zeros(9), only_last, np.eye(3).reshape(9)]])
    with np.errstate(all="ignore"):
        mo, me = oracle.inlier_moments(sc.src, sc.dst, H, THR2)
        mo_def, me_def, mag = P.moments(sc.src, sc.dst, H, THR2)
    assert np.array_equal(mo[:, 0], mo_def[:, 0])
    assert mo[0, 0] > n // 10 and mo[6, 0] == 0 and mo[7, 0] == 0 and mo[8, 0] >= 1
    assert np.all(np.abs(mo[:, 1:] - mo_def[:, 1:]) <= (math.ceil(n / 256) + 9) * EPS * mag)
    worst = 0.0
    for k in range(H.shape[0]):
        norm = np.linalg.norm(P.moment_matrix(mo_def[k]))
        err = abs(me[k] - me_def[k])
        if norm > 0:
            worst = max(worst, err / (EPS * norm))
        assert err <= MIN_EIG_FACTOR * EPS * norm, (k, me[k], me_def[k])
    print(f"n={n}: worst |min_eig - eigvalsh| / (2^-52 |M|_F) = {worst:.3g}")


def test_exact_threshold_points_sit_where_they_say(oracle):
    """The identity's forward error on per_label_numpy.exact_threshold_points is 4.0 exactly, just under and just over."""
    src, dst, kind = P.exact_threshold_points(40)
    d2 = oracle.residual_matrix(src, dst, np.eye(3).reshape(1, 9))[0]
    assert np.all(d2[kind == 0] == 4.0) and np.all(d2[kind < 0] < 4.0) and np.all(d2[kind > 0] > 4.0)
    assert dst[1, 0] == np.nextafter(2.0, 0) and d2[1] == np.nextafter(2.0, 0) * np.nextafter(2.0, 0)
    mo, me, _ = P.moments(src, dst, np.eye(3).reshape(1, 9), 4.0)
    assert mo[0, 0] == 40 and mo[0, 2] == 0 and mo[0, 4] == 0 and mo[0, 5] == 0


def test_same_bits_tells_zero_signs_and_infinities_apart():
    a = np.array([0.0, np.nan, np.inf, 1.0])
    assert P.same_bits(a, a.copy())
    assert P.same_bits(a, np.array([0.0, -np.nan, np.inf, 1.0]))
    assert not P.same_bits(a, np.array([-0.0, np.nan, np.inf, 1.0]))
    assert not P.same_bits(a, np.array([0.0, np.nan, np.nan, 1.0]))
    assert not P.same_bits(a, np.array([0.0, np.nan, -np.inf, 1.0]))
