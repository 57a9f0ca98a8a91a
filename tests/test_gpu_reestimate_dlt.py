"""The per-label N-point DLT estimator on the GPU (mh_set_estimator(MH_ESTIMATOR_DLT); csrc/reestimate_dlt.hip,
k_dlt_reestimate): every H against the twin (tests/reestimate_dlt_numpy.py::reestimate over refit_h_numpy.fit) BIT FOR BIT — the
standard k_refit_h meets with the same arithmetic — at the stride and membership edges of the match loop, the keep-on-failure
cases, what the entry points need under each estimator, the labeling step, the refitted winners of both greedy selections
(key 30) against a numpy greedy twin, and the sharded selection."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import reestimate_dlt_numpy as D
import refit_h_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

INVALID, NOT_SET = -2, -4
THR2 = 2.2 ** 2
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _code(mh, fn):
    with pytest.raises(mh.MultiHError) as ei:
        fn()
    return ei.value.code


def _label_counts(engine, nh):
    """The member counts the last re-estimation wrote (MH_BUF_LABEL_COUNTS)."""
    out = engine.label_counts()
    assert out.shape == (nh,) and out.dtype == np.int32
    return out


def _models(rng, nh):
    """Models a failed fit must keep: arbitrary finite doubles."""
    return np.ascontiguousarray(rng.normal(size=(nh, 9)))


def _check(engine, src, dst, labels, H_in):
    """mh_reestimate under "dlt" on these points, labels and models: H and the member counts against the twin."""
    nh = H_in.shape[0]
    engine.set_correspondences(src, dst)
    engine.set_estimator("dlt")
    engine.set_models(H_in)
    got = engine.reestimate(labels)
    want, counts = D.reestimate(src, dst, labels, H_in)
    assert np.array_equal(_bits(got), _bits(want)), np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
    assert np.array_equal(_bits(engine.get_models()), _bits(want))
    assert np.array_equal(_label_counts(engine, nh), counts)
    return want, counts


def _planes(rng, n, nh, noise=0.5):
    """n points, every one on the plane of its label (labels 0 .. nh-1 drawn uniformly)."""
    labels = rng.integers(0, nh, size=n).astype(np.int32)
    src = rng.uniform(0, 1000, size=(n, 2))
    dst = np.empty_like(src)
    for k in range(nh):
        m = labels == k
        if m.any():
            s, d, _, _ = R.plane_scene(rng, int(m.sum()), noise)
            src[m], dst[m] = s, d
    return src, dst, labels


# ---- 1. stride and membership edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh", [1, 3])
@pytest.mark.parametrize("n", [4, 5, 255, 256, 257, 513, 2048])
def test_stride_edges(engine, n, nh):
    rng = np.random.default_rng(1000 * nh + n)
    src, dst, labels = _planes(rng, n, nh)
    _, counts = _check(engine, src, dst, labels, _models(rng, nh))
    assert counts.sum() == n


def test_members_that_share_one_lane(engine):
    rng = np.random.default_rng(21)
    n = 1280
    src, dst, labels = _planes(rng, n, 2)
    lane = np.array([7, 263, 519, 775, 1031])
    labels[labels == 1] = 0
    labels[lane] = 1
    s, d, _, _ = R.plane_scene(rng, 5, 0.5)
    src[lane], dst[lane] = s, d
    want, counts = _check(engine, src, dst, labels, _models(rng, 2))
    assert counts.tolist() == [n - 5, 5]
    assert np.abs(R.unit_sign(want[1]) - R.fit_plain(src, dst, lane)).max() <= 1e-6


def test_four_members_three_members_and_foreign_labels(engine):
    rng = np.random.default_rng(22)
    n = 700
    src, dst, labels = _planes(rng, n, 1)
    perm = rng.permutation(n)
    labels[perm[:4]] = 1                                   # exactly 4: the smallest set that is fitted
    labels[perm[4:7]] = 2                                  # exactly 3: keeps its H
    labels[perm[7:60]] = -1
    labels[perm[60:90]] = 3                                # >= Nh
    labels[perm[90:100]] = 1 << 20
    s, d, _, _ = R.plane_scene(rng, 4, 0.0)
    src[perm[:4]], dst[perm[:4]] = s, d
    H_in = _models(rng, 3)
    want, counts = _check(engine, src, dst, labels, H_in)
    assert counts.tolist() == [n - 100, 4, 3]
    assert np.array_equal(_bits(want[2]), _bits(H_in[2])) and not np.array_equal(_bits(want[1]), _bits(H_in[1]))


def test_three_hundred_labels(engine):
    rng = np.random.default_rng(23)
    n, nh = 2048, 300
    src, dst, labels = _planes(rng, n, 6)
    labels = labels.astype(np.int32)
    # labels 6 .. 299 get 0 .. 3 members each, taken from the others: most labels stay under 4 members
    perm = rng.permutation(n)
    at = 0
    for k in range(6, nh):
        c = int(rng.integers(0, 4))
        labels[perm[at:at + c]] = k
        at += c
    H_in = _models(rng, nh)
    want, counts = _check(engine, src, dst, labels, H_in)
    small = counts < 4
    assert small.sum() >= 290 and (~small).sum() >= 6
    assert np.array_equal(_bits(want[small]), _bits(H_in[small]))


# ---- 2. failure cases ---------------------------------------------------------------------------------------------------------
def test_failed_fits_keep_their_models_and_leave_the_others_alone(engine):
    rng = np.random.default_rng(24)
    src, dst, labels = _planes(rng, 600, 5)
    # label 0: 3 members; label 2: all members the same point; label 3: a NaN coordinate in a member; label 5: no members
    zero = np.flatnonzero(labels == 0)
    labels[zero[3:]] = 1
    # (the same point 64 times, integer coordinates: the sums and the scale by 1 / 64 are exact, so the centroid is the point
    # itself, both mean distances are 0 and the scales are not finite.  Where the centroid rounds away from the point the
    # scales are finite, the fit is defined, and the kernel follows the twin there like anywhere else.)
    same = np.flatnonzero(labels == 2)
    labels[same[64:]] = 1
    same = same[:64]
    src[same], dst[same] = np.floor(src[same[0]]), np.floor(dst[same[0]])
    nan_at = np.flatnonzero(labels == 3)[5]
    H_in = _models(rng, 6)
    clean, _ = D.reestimate(src, dst, labels, H_in)        # before the NaN goes in
    dst[nan_at, 0] = np.nan
    want, counts = _check(engine, src, dst, labels, H_in)
    assert counts[0] == 3 and counts[5] == 0
    for k in (0, 2, 3, 5):
        assert np.array_equal(_bits(want[k]), _bits(H_in[k])), k
    for k in (1, 4):                                       # the NaN in label 3 leaves the other labels' results untouched
        assert np.array_equal(_bits(want[k]), _bits(clean[k])) and not np.array_equal(_bits(want[k]), _bits(H_in[k])), k


# ---- 2a. one fit, two kernels -------------------------------------------------------------------------------------------------
def _accepted_refit_scene(n):
    """A scene and a start whose first refit is accepted (checked with the twin, no GPU needed): n = 4 is the plane's own four
    points without noise, n = 257 has 30 % outliers and starts from a fit to eight of the plane's points."""
    rng = np.random.default_rng(7000 + n)
    outliers = int(0.3 * n) if n > 4 else 0
    src, dst, H_true, good = R.plane_scene(rng, n - outliers, 0.7 if n > 4 else 0.0, outliers=outliers)
    H_in = R.fit(src, dst, np.sort(rng.choice(np.flatnonzero(good), 8, replace=False))) if n > 4 else H_true
    return src, dst, H_in


@pytest.mark.parametrize("n", [4, 257])
def test_the_label_fit_is_the_refit_of_the_same_set(engine, n):
    """k_dlt_reestimate and k_refit_h run one fit (csrc/wg_fit.hpp): on labels = the inlier mask of H_in, the per-label
    estimator returns the nine doubles of mh_refit_homography's first, accepted, round, bit for bit."""
    src, dst, H_in = _accepted_refit_scene(n)
    why = []
    H_twin, _, _, acc_twin = R.refit(src, dst, H_in, THR2, 1, why)
    assert acc_twin == 1 and why == ["iterations"], (acc_twin, why)          # (a property of the scene, not of the engine)
    engine.set_correspondences(src, dst)
    _, mask, inliers, _ = engine.refit_homography(H_in, THR2, 0)
    H_refit, _, _, accepted = engine.refit_homography(H_in, THR2, 1)
    assert accepted == 1 and inliers >= 4
    labels = np.where(mask != 0, 0, -1).astype(np.int32)
    engine.set_estimator("dlt")
    engine.set_models(_models(np.random.default_rng(n), 1))
    got = engine.reestimate(labels)
    assert _label_counts(engine, 1).tolist() == [inliers]
    assert np.array_equal(_bits(got[0]), _bits(H_refit)), (got[0], H_refit)
    assert np.array_equal(_bits(got[0]), _bits(H_twin))


# ---- 3. no epipolar geometry needed -------------------------------------------------------------------------------------------
def _motions(n):
    if n not in _cache:
        _cache[n] = D.three_motions(n)
    return _cache[n]


def test_no_epipolar_geometry_needed(mh, engine):
    sc = _motions(600)
    engine.set_correspondences(sc.src, sc.dst)             # neither affinities nor mh_set_epipolar
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    start = np.full(sc.n, -1, np.int32)
    for name in ("haf", "3pt"):
        engine.set_estimator(name)
        engine.set_models(sc.H_true)
        assert _code(mh, lambda: engine.reestimate(sc.gt_label)) == NOT_SET, name
        assert _code(mh, lambda: engine.labeling_step(False, start)) == NOT_SET, name
    engine.set_estimator("dlt")
    engine.set_models(sc.H_true)
    engine.data_cost(fetch=False)
    H = engine.reestimate(sc.gt_label)
    assert np.array_equal(_bits(H), _bits(D.reestimate(sc.src, sc.dst, sc.gt_label, sc.H_true)[0]))
    for k in range(3):                                     # 0.5 px of noise per coordinate: an RMS of 0.71 px on the members
        m = sc.gt_label == k
        assert np.sqrt(R.d2_of(sc.src[m], sc.dst[m], H[k]).mean()) < 1.0, k
    assert _code(mh, lambda: engine.expand()) == NOT_SET   # the models changed: the data cost is stale
    engine.data_cost(fetch=False)
    engine.expand()
    engine.labeling_step(False, start)


# ---- 4. the labeling step -----------------------------------------------------------------------------------------------------
def test_labeling_step_under_dlt(engine):
    sc = _motions(600)
    engine.set_correspondences(sc.src, sc.dst)
    engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    engine.set_estimator("dlt")
    engine.set_models(sc.H_true)
    engine.data_cost(fetch=False)
    lab_gco, energy, cycles = engine.expand()
    engine.set_models(sc.H_true)
    lab, en, cyc = engine.labeling_step(False, np.full(sc.n, -1, np.int32))
    assert np.array_equal(lab, lab_gco - 1) and en == energy and cyc == cycles
    assert all((lab == k).sum() >= 50 for k in range(3))
    want, counts = D.reestimate(sc.src, sc.dst, lab, sc.H_true)
    assert np.array_equal(_bits(engine.get_models()), _bits(want))
    assert np.array_equal(_label_counts(engine, 3), counts)


# ---- 5. key 30 ----------------------------------------------------------------------------------------------------------------
N_SEL, M_SEL, NEED, MAX_MODELS, SEED = 300, 64, 8, 8, 6


def _selection_scene():
    """300 points: planes of 170 and 90 correspondences at 0.5 px noise, 40 uniform outliers."""
    if "sel" not in _cache:
        rng = np.random.default_rng(31)
        a = R.plane_scene(rng, 170, 0.5)
        b = R.plane_scene(rng, 90, 0.5, outliers=40)
        src, dst = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
        perm = rng.permutation(N_SEL)
        _cache["sel"] = (np.ascontiguousarray(src[perm]), np.ascontiguousarray(dst[perm]))
    return _cache["sel"]


def _batch(engine, src, dst):
    engine.set_correspondences(src, dst)
    engine.propose_dlt4(SEED, 0, M_SEL)
    return engine.get_models()


def test_refitted_winners_by_count(engine):
    src, dst = _selection_scene()
    engine.set_estimator("dlt")
    engine.set_tuning(30, 1)
    batch = _batch(engine, src, dst)
    H, counters, counts, mask = engine.select_greedy(THR2, NEED, MAX_MODELS, np.ones(N_SEL, np.uint8))
    H_t, idx_t, cnt_t, _, mask_t = D.select_greedy(src, dst, batch, THR2, NEED, MAX_MODELS, rank_by="count")
    assert len(idx_t) >= 2                                               # (a property of the twin on this scene, not of the engine)
    assert any(not np.array_equal(_bits(h), _bits(batch[i])) for h, i in zip(H_t, idx_t)), "no refit was taken"
    assert len(counters) == len(idx_t)
    assert np.array_equal(counters, idx_t) and np.array_equal(counts, cnt_t) and np.array_equal(mask, mask_t)
    assert np.array_equal(_bits(H), _bits(H_t))


def test_refitted_winners_by_weight(engine):
    src, dst = _selection_scene()
    engine.set_estimator("dlt")
    engine.set_tuning(30, 1)
    batch = _batch(engine, src, dst)
    H, counters, counts, weights, mask = engine.select_greedy_msac(THR2, NEED, MAX_MODELS, np.ones(N_SEL, np.uint8))
    H_t, idx_t, cnt_t, wgt_t, mask_t = D.select_greedy(src, dst, batch, THR2, NEED, MAX_MODELS, rank_by="weight")
    assert len(idx_t) >= 2
    assert len(counters) == len(idx_t)
    assert np.array_equal(counters, idx_t) and np.array_equal(counts, cnt_t) and np.array_equal(weights, wgt_t)
    assert np.array_equal(mask, mask_t)
    assert np.array_equal(_bits(H), _bits(H_t))


def test_without_key_30_the_estimator_changes_nothing(engine):
    src, dst = _selection_scene()
    engine.set_tuning(30, 0)
    out = {}
    for name in ("haf", "dlt"):
        engine.set_estimator(name)
        _batch(engine, src, dst)
        out[name] = engine.select_greedy(THR2, NEED, MAX_MODELS, np.ones(N_SEL, np.uint8))
        _batch(engine, src, dst)
        out[name + "w"] = engine.select_greedy_msac(THR2, NEED, MAX_MODELS, np.ones(N_SEL, np.uint8))
    for a, b in (("haf", "dlt"), ("hafw", "dltw")):
        assert len(out[a][1]) >= 2
        assert np.array_equal(_bits(out[a][0]), _bits(out[b][0]))
        assert all(np.array_equal(x, y) for x, y in zip(out[a][1:], out[b][1:]))


# ---- 6. sharded ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_selection_with_dlt_refits(mh, engine):
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "reestimate_dlt_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)          # a stranded rank would run into these
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda d: d["rank"])
    assert [d["rank"] for d in recs] == [0, 1]
    # the single-rank call over the same 600 hypotheses
    sc = mh.synth.make_scene(600, 3, seed=99, with_neighbours=False)
    engine.set_params(2.6, 2.5, 0.005, 0.5, 20)
    engine.set_correspondences(sc.src, sc.dst)
    engine.set_estimator("dlt")
    engine.set_tuning(30, 1)
    engine.propose_dlt4(77, 0, 600)
    batch = engine.get_models()
    H, counters, counts, _ = engine.select_greedy(6.25, 20, 8, np.ones(sc.n, np.uint8))
    assert len(counters) >= 2
    assert any(not np.array_equal(_bits(h), _bits(batch[i])) for h, i in zip(H, counters)), "no refit was taken"
    for rr in recs:
        for name in ("dlt_refit", "dlt_again"):
            assert rr[name]["ok"], rr[name]
            assert rr[name]["counters"] == counters.tolist() and rr[name]["counts"] == counts.tolist(), name
            assert rr[name]["H"] == H.view(np.uint64).tolist(), name
        # one rank on "dlt", the other on "3pt": both leave with the mode-mismatch error
        assert not rr["mixed"]["ok"] and rr["mixed"]["code"] == INVALID, rr["mixed"]
        assert "the estimator (mh_set_estimator)" in rr["mixed"]["msg"], rr["mixed"]


# ---- 7. mh_set_estimator ------------------------------------------------------------------------------------------------------
def test_set_estimator(mh, engine):
    assert engine.lib.mh_set_estimator(engine._h, 3) == INVALID
    assert engine.lib.mh_set_estimator(engine._h, -1) == INVALID
    src, dst, labels = _planes(np.random.default_rng(41), 300, 2)
    engine.set_estimator("dlt")
    engine.set_correspondences(src, dst)                   # sticky: the estimator survives new correspondences
    H_in = _models(np.random.default_rng(42), 2)
    engine.set_models(H_in)
    got = engine.reestimate(labels)                        # (would answer MH_ERR_NOT_SET under "haf" and "3pt")
    assert np.array_equal(_bits(got), _bits(D.reestimate(src, dst, labels, H_in)[0]))
