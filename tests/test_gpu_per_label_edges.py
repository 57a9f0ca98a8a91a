"""The per-label and per-model reduction kernels at their membership and chunk edges.

k_haf_reestimate reads its labels 32 per lane and trip (8192 points) and visits the matches four at a time; k_moments strides
by 2048 points; the 3-point fit chooses its member form at 8192 block counts and ranks every point inside its block of 256;
k_inliers_of_model and k_moments test d2 < thr2 strictly; k_haf_point writes inf and NaN rows for degenerate correspondences.
Every case here sits on one of those edges (tests/per_label_numpy.py makes the label patterns and the exact-threshold
points) and is held to the oracle: bit for bit where the oracle sums in the kernel's order (HAF, moments, inliers, per-point
fits), to the 1e-6 of tests/test_gpu_points_only.py where it does not (the 3-point fit).  tests/test_per_label_cpu.py holds
the oracle itself to the plain definitions on the same patterns.  Every case uses the scene's own F and epipole."""
import functools

import numpy as np
import pytest

import per_label_numpy as P
from test_gpu_points_only import _label_counts, _rel_frob

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]

THR2_EXACT = 4.0             # the threshold the exact-threshold points are built for


@functools.lru_cache(maxsize=None)
def _scene(synth, n, seed):
    sc = synth.make_scene(n, 3, seed=seed, with_neighbours=False)
    for a in (sc.src, sc.dst, sc.aff, sc.gt_label, sc.H_true, sc.F, sc.e2):
        a.setflags(write=False)
    return sc


def _labels(sc, kind, Nh, seed):
    """kind "edge": edge_labels; "one": every point in label 1 (of 3); "none": every point -1; "all0": every point in label 0."""
    n = sc.n
    if kind == "edge":
        return P.edge_labels(n, Nh, np.random.default_rng(seed), sc.gt_label)
    value = {"one": 1, "none": -1, "all0": 0}[kind]
    return np.full(n, value, dtype=np.int32), {}


def _initial_models(sc, Nh, seed):
    rng = np.random.default_rng(seed + 1000)
    return sc.H_true[np.arange(Nh) % 3] * (1.0 + rng.normal(0, 1e-3, (Nh, 9)))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- HAF re-estimation -----------------------------------------------------------------------------------------------

HAF_CASES = [(n, kind, 3, 0.0) for n in (1, 3, 255, 256) for kind in ("one", "none")]
HAF_CASES += [(n, "edge", 12, 0.0) for n in (257, 8191, 8192, 8193, 16641)]
HAF_CASES += [(8193, "all0", 1, 0.0),            # one model that owns every point: every lane's mask is full in the first trip
              (16641, "edge", 130, 0.0),         # many labels, most of them small
              (8193, "edge", 12, 5000.0)]        # both images shifted by 5000 px: entries of A^T A reach 1e14


@pytest.mark.parametrize("n,kind,Nh,shift", HAF_CASES)
def test_haf_reestimate_at_membership_edges(engine, synth, oracle, n, kind, Nh, shift):
    sc = _scene(synth, n, 40 + n % 7)
    src, dst = sc.src + shift, sc.dst + shift
    labels, where = _labels(sc, kind, Nh, n)
    if kind == "edge":
        assert set("abcdi") <= set(where) and len(where["stray"]) == 4
        if n > 8192:
            assert set("efh") <= set(where)
        if n == 16641:
            assert set(P.PATTERNS) <= set(where)
            lane7 = P.members_of(labels, where["e"])
            assert np.array_equal(lane7[:32], 7 + 256 * np.arange(32)) and lane7.size > 32      # a full mask, then a remainder
            assert np.count_nonzero(labels == where["h"]) == 256
    H0 = _initial_models(sc, Nh, n)
    engine.set_correspondences(src, dst, sc.aff)
    engine.set_epipolar(sc.F, sc.e2)
    engine.set_models(H0)
    H = engine.reestimate(labels)
    cnt = _label_counts(engine, Nh)
    engine.set_models(H0)
    H_again = engine.reestimate(labels)
    with np.errstate(all="ignore"):
        H_ref, cnt_ref = oracle.haf_reestimate(src, dst, sc.aff, labels, H0, sc.F, sc.e2)
    assert np.array_equal(cnt, P.in_range_counts(labels, Nh))
    assert np.array_equal(cnt, cnt_ref)
    empty = cnt == 0
    if kind in ("edge", "one", "none"):
        assert empty.any()
    assert np.array_equal(_bits(H[empty]), _bits(H0[empty])), "a label without members keeps its H bit for bit"
    fin = np.isfinite(H_ref)
    assert np.array_equal(_bits(H[fin]), _bits(H_ref[fin])), "finite entries differ from the oracle's"
    assert np.array_equal(np.isnan(H), np.isnan(H_ref)) and np.array_equal(np.isinf(H), np.isinf(H_ref))
    assert P.same_bits(H, H_ref)
    assert H.tobytes() == H_again.tobytes(), "two runs from the same models must give the same bits"
    if kind != "none":
        assert not np.array_equal(H[~empty], H0[~empty])


# ---- 3-point re-estimation --------------------------------------------------------------------------------------------

def _run_3pt(engine, oracle, sc, labels, Nh, H0):
    """One point-only re-estimation held to the oracle; returns (H, counts, the labels that were fitted)."""
    engine.set_correspondences(sc.src, sc.dst)            # no affinities
    engine.set_epipolar(sc.F, sc.e2)
    engine.set_estimator("3pt")
    engine.set_models(H0)
    H = engine.reestimate(labels)
    cnt = _label_counts(engine, Nh)
    engine.set_models(H0)
    H_again = engine.reestimate(labels)
    assert H.tobytes() == H_again.tobytes(), "two runs must be bit-identical"
    assert np.array_equal(cnt, P.in_range_counts(labels, Nh))
    fitted = []
    for l in range(Nh):
        m = P.members_of(labels, l)
        ref, ok = P.fit_3pt_members(sc.src, sc.dst, m, sc.F) if m.size >= 3 else (None, False)
        if not ok:
            assert np.array_equal(_bits(H[l]), _bits(H0[l])), f"label {l} ({m.size} members) keeps its H"
            continue
        assert _rel_frob(H[l], ref)[0] <= 1e-6, (l, m.size, _rel_frob(H[l], ref))
        fitted.append(l)
    return H, cnt, fitted


@pytest.mark.parametrize("n,kind,Nh", [(3, "all0", 1), (257, "edge", 4), (16641, "edge", 12)])
def test_3pt_reestimate_at_membership_edges(engine, synth, oracle, n, kind, Nh):
    """n = 3: one block, one count, exactly the minimal sample.  257 x 4: a scan over 8 counts and a last block of one point.
    16 641 x 12: every pattern, a block rank of 255, the compacted form over 792 counts."""
    sc = _scene(synth, n, 40 + n % 7)
    labels, where = _labels(sc, kind, Nh, n)
    if n == 16641:
        assert set(P.PATTERNS) <= set(where) and len(where["stray"]) == 4
        assert np.count_nonzero(labels == where["h"]) == 256
    H, cnt, fitted = _run_3pt(engine, oracle, sc, labels, Nh, _initial_models(sc, Nh, n))
    assert fitted, "no label was fitted"
    if n == 16641:
        assert set(fitted) == {0, 1, 2} | {where[p] for p in "defghi"}


def test_3pt_forms_on_both_sides_of_the_compaction_limit(engine, synth, oracle):
    """8200 points are 33 blocks: 248 labels make 8184 block counts (compacted member lists), 249 make 8217 (the match loop).
    The same label array serves both runs (label 248 is one more stray value for the first), so the first 248 labels have the
    same members under both forms."""
    n = 8200
    sc = _scene(synth, n, 45)
    labels, where = _labels(sc, "edge", 249, n)
    assert set("abcdefhi") <= set(where) and len(where["stray"]) == 4
    assert P.members_of(labels, 248).size >= 3, "label 248 should have members for the second run to fit"
    H0 = _initial_models(sc, 249, n)
    assert 248 * 33 <= 8192 < 249 * 33
    H_c, cnt_c, fit_c = _run_3pt(engine, oracle, sc, labels, 248, H0[:248])
    H_m, cnt_m, fit_m = _run_3pt(engine, oracle, sc, labels, 249, H0)
    assert np.array_equal(cnt_c, cnt_m[:248])
    assert fit_c == [l for l in fit_m if l < 248] and len(fit_c) > 150
    assert np.all(_rel_frob(H_c[fit_c], H_m[fit_c]) <= 1e-6)
    kept = np.setdiff1d(np.arange(248), fit_c)
    assert np.array_equal(_bits(H_c[kept]), _bits(H_m[kept]))


# ---- moments, inlier labels: points whose error sits exactly at the threshold --------------------------------------------

LONELY_SRC, LONELY_DST = (123.5, 77.25), (-3000.5, -4000.25)


def _threshold_scene(synth, n, k):
    """n points: scene points, then 3 k exact-threshold points (per_label_numpy.exact_threshold_points), then one point whose
    target lies far outside the image (the only inlier of the model that maps everything onto that target)."""
    k = min(k, (n - 1) // 3)
    n_scene = n - 3 * k - 1
    sc = _scene(synth, max(n_scene, 3), 50 + n % 5)
    es, ed, kind = P.exact_threshold_points(k)
    src = np.concatenate([sc.src[:n_scene], es, [LONELY_SRC]])
    dst = np.concatenate([sc.dst[:n_scene], ed, [LONELY_DST]])
    kinds = np.concatenate([np.full(n_scene, 9), kind, [9]])
    return sc, src, dst, kinds


@pytest.mark.parametrize("M", [1, 17])
@pytest.mark.parametrize("n", [1, 255, 256, 2047, 2048, 2049, 4100])
def test_moments_at_chunk_and_threshold_edges(engine, synth, oracle, n, M):
    sc, src, dst, kinds = _threshold_scene(synth, n, 12)
    identity = np.eye(3).reshape(9)
    only_last = np.array([0, 0, LONELY_DST[0], 0, 0, LONELY_DST[1], 0, 0, 1.0])
    far = np.array([1, 0, 1e5, 0, 1, 1e5, 0, 0, 1.0])
    if M == 1:
        H = (only_last if n == 1 else identity).reshape(1, 9)
    else:
        rng = np.random.default_rng(n)
        near = sc.H_true[np.arange(10) % 3] * (1.0 + rng.normal(0, 2e-4, (10, 9)))
        H = np.concatenate([sc.H_true, [far, np.zeros(9), only_last, identity], near])
    assert H.shape[0] == M
    engine.set_correspondences(src, dst)
    engine.set_models(H)
    mo, me = engine.inlier_moments(THR2_EXACT)
    with np.errstate(all="ignore"):
        mo_ref, me_ref = oracle.inlier_moments(src, dst, H, THR2_EXACT)
        inl = oracle.residual_matrix(src, dst, H) < THR2_EXACT
    # the oracle's own decisions are the ones the cases are built for
    i_id = M - 1 if M == 1 else 6
    if n > 1:
        assert not inl[i_id, kinds == 0].any() and not inl[i_id, kinds == 1].any() and inl[i_id, kinds == -1].all()
        assert (kinds == -1).sum() >= 1
    if M == 17:
        assert mo_ref[3, 0] == 0 and mo_ref[4, 0] == 0                 # far off; the zero H (every d2 NaN)
        assert mo_ref[5, 0] == 1 and inl[5, n - 1]                       # its only inlier is point n - 1
        if n >= 255:
            assert mo_ref[:3, 0].max() > n // 10
    assert np.array_equal(mo_ref[:, 0], inl.sum(axis=1))
    assert np.array_equal(mo[:, 0], mo_ref[:, 0])
    assert np.array_equal(_bits(mo), _bits(mo_ref)), "moment sums differ from the oracle's"
    assert P.same_bits(me, me_ref), (me, me_ref)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_inlier_labels_at_the_threshold(engine, synth, oracle, n):
    sc, src, dst, kinds = _threshold_scene(synth, n, 20)
    k = int(np.flatnonzero(kinds == -1)[1]) if n > 1 else 0          # the point the inf-producing model is built on (x != 0)
    nan_model = np.full(9, np.nan)
    inf_model = np.array([1, 0, 0, 0, 1, 0, 1, 0, -src[k, 0]])       # s = x - x_k: 0 at point k
    H = np.concatenate([sc.H_true, [nan_model, np.zeros(9), inf_model, np.eye(3).reshape(9)]])
    m = H.shape[0]
    rng = np.random.default_rng(n)
    before = rng.integers(-1, 7, size=n).astype(np.int32)
    engine.set_correspondences(src, dst)
    engine.set_models(H)
    with np.errstate(all="ignore"):
        d2 = oracle.residual_matrix(src, dst, H)
    assert np.isnan(d2[3]).all() and np.isnan(d2[4]).all() and not d2[5, k] < THR2_EXACT and not np.isfinite(d2[5, k])
    if n > 1:
        assert np.all(d2[m - 1, kinds == 0] == THR2_EXACT) and np.all(d2[m - 1, kinds == -1] < THR2_EXACT)
    for idx in (m - 1, 3, 4, 5, 0):
        want = np.where(d2[idx] < THR2_EXACT, -3, before).astype(np.int32)
        got = engine.inliers_of_model(idx, THR2_EXACT, -3, before)
        assert np.array_equal(got, want), idx
        assert np.array_equal(engine.inliers_of_homography(H[idx], THR2_EXACT, -3, before), want), idx
        if idx in (3, 4):
            assert np.array_equal(got, before), "a model whose every d2 is NaN touches no label"
        if idx == 5:
            assert got[k] == before[k]
    if n > 1:
        got = engine.inliers_of_model(m - 1, THR2_EXACT, -3, before)
        assert np.all(got[kinds == -1] == -3) and np.array_equal(got[kinds == 0], before[kinds == 0])


# ---- per-point homographies ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 256, 257])
def test_local_homographies_with_degenerate_rows(engine, synth, oracle, n):
    sc = _scene(synth, max(n, 3), 60 + n % 3)
    src, dst, aff = sc.src[:n].copy(), sc.dst[:n].copy(), sc.aff[:n].copy()
    aff[0] = 0.0                                           # a zero affinity
    if n > 1:
        aff[1] = [1.0, 2.0, 2.0, 4.0]                      # a singular affinity
        dst[2] = sc.e2                                     # the target exactly at the epipole
        src[4], dst[4], aff[4] = src[3], dst[3], aff[3]    # a duplicate of another row
        aff[n - 1] = 0.0
        dst[n - 1] = sc.e2                                 # the last row: both at once
    else:
        dst[0] = sc.e2
    engine.set_correspondences(src, dst, aff)
    engine.set_epipolar(sc.F, sc.e2)
    H, feat = engine.local_homographies(0.005)
    with np.errstate(all="ignore"):
        H_ref, feat_ref = oracle.haf_point(src, dst, aff, sc.F, sc.e2, 0.005)
    ok = np.isfinite(H_ref).all(axis=1) & np.isfinite(feat_ref).all(axis=1)
    assert not ok.all(), "no degenerate row came out non-finite: the case would be vacuous"
    if n > 1:
        assert ok.sum() >= n - 6
        assert np.array_equal(_bits(H[4]), _bits(H[3])) and np.array_equal(_bits(feat[4]), _bits(feat[3]))
    assert np.array_equal(_bits(H[ok]), _bits(H_ref[ok]))
    assert np.array_equal(_bits(feat[ok]), _bits(feat_ref[ok]))
    assert P.same_bits(H, H_ref), "non-finite rows: NaN in other places, or other bits where not NaN"
    assert P.same_bits(feat, feat_ref)
