"""The point-only route: correspondences without affinities.

mh_set_estimator(MH_ESTIMATOR_3PT) replaces the per-label HAF fit with GetHomography3PT's least squares over each label's
members (csrc/reestimate3pt.hip) in mh_reestimate, mh_labeling_step and the refitted winners of mh_select_greedy;
mh_refine_points runs the Hartley-Sturm correction of mh_refine_correspondences alone; MultiH::Process(src, dst) and the
harness's --points option put them together.  Each check is held against the oracle (tests/oracle_lib.py) or the
harness's own ground truth."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]

THR = 2.2
THR2 = THR * THR
LAM = 0.5


def _scaled(H):
    H = np.asarray(H, dtype=np.float64).reshape(-1, 9)
    return H / H[:, 8:9]


def _rel_frob(a, b):
    a, b = _scaled(a), _scaled(b)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def _f_compatibility(H, F):
    """|H^T F + F^T H| relative to |F| |H| per model: 0 for a homography induced by a plane of the epipolar geometry F."""
    Fm = np.asarray(F, dtype=np.float64).reshape(3, 3)
    out = []
    for h in np.asarray(H).reshape(-1, 9):
        Hm = h.reshape(3, 3)
        S = Hm.T @ Fm + Fm.T @ Hm
        out.append(np.linalg.norm(S) / (np.linalg.norm(Fm) * np.linalg.norm(Hm)))
    return np.array(out)


def _points_only_engine(engine, sc, neighbours=False):
    engine.set_correspondences(sc.src, sc.dst)            # no affinities
    engine.set_epipolar(sc.F, sc.e2)
    if neighbours:
        engine.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
    engine.set_estimator("3pt")


def _label_counts(engine, nh):
    """The member counts the last re-estimation wrote (MH_BUF_LABEL_COUNTS), copied by the HIP runtime the engine has loaded."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    ptr, nbytes = engine.device_buffer(6)
    assert nbytes == 4 * nh
    out = np.empty(nh, dtype=np.int32)
    engine.synchronize()
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), 4 * nh, 2) == 0      # hipMemcpyDeviceToHost
    return out


def _special_labels(sc, rng):
    """Ground-truth labels plus five extra labels: 0, 1, 2 and 3 members, and a tight cluster of 6 (nearly degenerate)."""
    lab = sc.gt_label.astype(np.int32).copy()
    K = sc.H_true.shape[0]
    plane0 = np.flatnonzero(lab == 0)
    take = rng.choice(plane0, size=6, replace=False)
    lab[take[:1]] = K + 1                                  # 1 member
    lab[take[1:3]] = K + 2                                 # 2 members
    lab[take[3:6]] = K + 3                                 # 3 members
    plane1 = np.flatnonzero(lab == 1)
    c = plane1[0]
    d = np.sum((sc.src[plane1] - sc.src[c]) ** 2, axis=1)
    lab[plane1[np.argsort(d)[:6]]] = K + 4                 # the 6 nearest points of plane 1: a small, nearly degenerate patch
    return lab, K + 5                                      # label K: no members


def test_3pt_reestimate_matches_the_host_fit_and_keeps_small_labels(mh, engine, oracle):
    sc = mh.synth.make_scene(6000, 4, seed=31, with_neighbours=False)
    rng = np.random.default_rng(31)
    lab, Nh = _special_labels(sc, rng)
    H0 = np.concatenate([sc.H_true, sc.H_true[rng.integers(0, 4, Nh - 4)] * (1 + rng.normal(0, 1e-3, (Nh - 4, 9)))])
    _points_only_engine(engine, sc)
    engine.set_models(H0)
    H = engine.reestimate(lab)
    engine.set_models(H0)
    H_again = engine.reestimate(lab)
    assert np.array_equal(H.view(np.uint64), H_again.view(np.uint64)), "two runs must be bit-identical"
    assert np.array_equal(_label_counts(engine, Nh), np.bincount(lab[lab >= 0], minlength=Nh))
    fitted = 0
    for l in range(Nh):
        m = np.flatnonzero(lab == l)
        if m.size < 3:
            assert np.array_equal(H[l].view(np.uint64), H0[l].view(np.uint64)), f"label {l} ({m.size} members) keeps its H"
            continue
        ref, ok = oracle.homography_3pt(sc.src[m], sc.dst[m], sc.F, refine=False)
        if not ok:
            assert np.array_equal(H[l].view(np.uint64), H0[l].view(np.uint64)), f"label {l}: fit not finite, H kept"
            continue
        assert _rel_frob(H[l], ref)[0] <= 1e-6, (l, m.size, _rel_frob(H[l], ref))
        fitted += 1
    assert fitted == Nh - 3                                # the four planes, the 3-member and the 6-member label
    assert np.all(_f_compatibility(H[:4], sc.F) <= 1e-9), _f_compatibility(H[:4], sc.F)
    # the planes' refits are close to the truth
    assert np.all(_rel_frob(H[:4], sc.H_true) <= 1e-2)


def test_3pt_reestimate_with_many_labels(mh, engine, oracle):
    """Hundreds of labels (the reference's route at 20 000 points carries 540): every label its own member list."""
    sc = mh.synth.make_scene(20000, 10, seed=32, with_neighbours=False)
    rng = np.random.default_rng(32)
    Nh = 540
    lab = rng.integers(-1, Nh, size=sc.n).astype(np.int32)
    lab[sc.gt_label >= 0] = sc.gt_label[sc.gt_label >= 0]      # the planes keep their points; the rest is spread over labels
    H0 = np.tile(sc.H_true, (Nh // 10, 1))
    _points_only_engine(engine, sc)
    engine.set_models(H0)
    H = engine.reestimate(lab)
    assert np.array_equal(_label_counts(engine, Nh), np.bincount(lab[lab >= 0], minlength=Nh))
    for l in list(range(10)) + list(rng.choice(np.arange(10, Nh), 20, replace=False)):
        m = np.flatnonzero(lab == l)
        ref, ok = oracle.homography_3pt(sc.src[m], sc.dst[m], sc.F, refine=False)
        if m.size >= 3 and ok:
            assert _rel_frob(H[l], ref)[0] <= 1e-6, (l, m.size)
        else:
            assert np.array_equal(H[l].view(np.uint64), H0[l].view(np.uint64)), l


def test_labeling_step_under_3pt_without_affinities(mh, engine, oracle):
    sc = mh.synth.make_scene(3000, 3, seed=33)
    _points_only_engine(engine, sc, neighbours=True)
    H = sc.H_true * (1.0 + np.random.default_rng(33).normal(0, 1e-4, size=sc.H_true.shape))
    engine.set_models(H)
    lab, energy, cycles = engine.labeling_step(False, np.full(sc.n, -1, dtype=np.int32))
    cost = oracle.data_cost(sc.src, sc.dst, H, LAM, THR2)
    want_lab, want_e, want_cyc, _ = oracle.expand(cost, sc.hit_rowptr, sc.hit_col, oracle.potts(LAM))
    assert energy == want_e and cycles == want_cyc
    assert np.array_equal(lab, want_lab - 1)
    Hg = engine.get_models()
    for l in range(H.shape[0]):
        m = np.flatnonzero(lab == l)
        if m.size < 3:
            assert np.array_equal(Hg[l], H[l])
            continue
        ref, ok = oracle.homography_3pt(sc.src[m], sc.dst[m], sc.F, refine=False)
        assert ok and _rel_frob(Hg[l], ref)[0] <= 1e-6, l
    # the HAF estimator without affinities still refuses, as before
    engine.set_estimator("haf")
    engine.set_models(H)
    with pytest.raises(mh.MultiHError) as ex:
        engine.labeling_step(False, np.full(sc.n, -1, dtype=np.int32))
    assert ex.value.code == -4


def test_selection_refit_under_3pt_without_affinities(mh, engine, oracle):
    sc = mh.synth.make_scene(5000, 4, seed=34, with_neighbours=False)
    _points_only_engine(engine, sc)
    engine.propose_dlt4(34, 0, 4000)
    proposals = engine.get_models()
    engine.set_tuning(30, 1)
    Hs, counters, counts, _ = engine.select_greedy(THR2, 20, 16)
    assert Hs.shape[0] >= 4
    mask = np.ones(sc.n, dtype=np.uint8)
    refitted = 0
    for k in range(Hs.shape[0]):
        # the selected model (refit or hypothesis) explains at least as many of the points left as the hypothesis did
        got = int(oracle.score(sc.src, sc.dst, Hs[k][None], THR2, mask=mask)[0])
        assert got >= counts[k], (k, got, counts[k])
        if not np.array_equal(Hs[k], proposals[counters[k]]):
            refitted += 1
            assert _f_compatibility(Hs[k], sc.F)[0] <= 1e-9
        with np.errstate(all="ignore"):
            d2 = oracle.residual_matrix(sc.src, sc.dst, Hs[k][None])[0]
        mask[(mask != 0) & (d2 < THR2)] = 0
    assert refitted >= 1
    # the HAF refit without affinities: MH_ERR_NOT_SET, as before
    engine.set_estimator("haf")
    with pytest.raises(mh.MultiHError) as ex:
        engine.select_greedy(THR2, 20, 16)
    assert ex.value.code == -4


def test_refine_points_is_step_one_of_refine_correspondences(mh, engine, oracle):
    sc = mh.synth.make_scene(4000, 3, seed=35, with_neighbours=False)
    rng = np.random.default_rng(35)
    in_mask = (rng.random(sc.n) > 0.1).astype(np.uint8)
    engine.set_correspondences(sc.src, sc.dst, sc.aff)
    e1, e2 = engine.epipoles(sc.F)
    keep, out = engine.refine_points(sc.F, e1, e2, in_mask)
    reason = engine.refine_reasons()
    keep_o, out_o, reason_o = oracle.refine_points(sc.src, sc.dst, sc.aff, sc.F, e1, e2, in_mask, with_reasons=True)
    assert np.any(reason_o == 3) and np.any(reason_o == 0) and np.any(reason_o == 1)
    kept = reason_o == 0
    assert np.array_equal(out[kept].view(np.uint64), out_o[kept, :4].view(np.uint64))
    for r in (1, 2):
        assert np.array_equal(reason[reason_o == r], reason_o[reason_o == r])
    assert np.all(reason[reason_o == 3] == 0) and np.all(keep[reason_o == 3] == 1)
    assert np.array_equal(keep, (reason == 0).astype(np.uint8))
    # the same without affinities on the engine
    engine.set_correspondences(sc.src, sc.dst)
    keep2, out2 = engine.refine_points(sc.F, e1, e2, in_mask)
    assert np.array_equal(keep2, keep) and np.array_equal(out2.view(np.uint64), out.view(np.uint64))
    assert np.array_equal(engine.refine_reasons(), reason)
    with pytest.raises(mh.MultiHError):
        engine.refine_correspondences(sc.F, e1, e2, in_mask)       # that one still needs the affinities


# ---- the whole route through the harness ---------------------------------------------------------------------------

def _harness(mh):
    return os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")


def _run(mh, rows, tmp_path, name, extra=(), timeout=40):
    corr = tmp_path / f"{name}.txt"
    np.savetxt(corr, rows, fmt="%.17g")
    out = tmp_path / f"{name}.out"
    r = subprocess.run([_harness(mh), str(corr), str(out), *extra], capture_output=True, text=True, timeout=timeout)
    return r, out


def _labels_on_the_input(sc, out):
    """The result rows are the points Process() kept (refined: moved by a fraction of a pixel) unless every input row is
    there; each is taken back to its input row by its nearest source point.  Rows that are not there count as outliers."""
    res = np.loadtxt(out, ndmin=2)
    assert res.shape[1] == 5, "x1 y1 x2 y2 label"
    full = np.full(sc.n, -1, dtype=np.int64)
    if res.shape[0] == sc.n:
        full[:] = res[:, 4]
        return full, res
    for a in range(0, res.shape[0], 512):
        q = res[a:a + 512, :2]
        d = ((q[:, None, :] - sc.src[None, :, :]) ** 2).sum(-1)
        full[np.argmin(d, axis=1)] = res[a:a + 512, 4]
    return full, res


@pytest.mark.parametrize("n,planes,seed", [(5000, 3, 1234), (20000, 10, 1234)])
def test_harness_points_route_recovers_the_planes(mh, tmp_path, n, planes, seed):
    sc = mh.synth.make_scene(n, planes, seed=seed, with_neighbours=False)
    rows = np.concatenate([sc.src, sc.dst], axis=1)
    r, out = _run(mh, rows, tmp_path, "a", ["--points"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    full, res = _labels_on_the_input(sc, out)
    found = len(set(int(v) for v in res[:, 4]) - {-1})
    ari = mh.synth.adjusted_rand_index(full, sc.gt_label)
    print(f"[points-only] n={n} planes={planes}: {found} planes found, ARI {ari:.4f}")
    assert abs(found - planes) <= 1, (found, planes, ari)
    assert ari >= 0.9, (found, ari)
    if n == 5000:
        r2, out2 = _run(mh, rows, tmp_path, "b", ["--points"])
        assert r2.returncode == 0
        assert open(out).read() == open(out2).read(), "two runs must write the same file"


def test_harness_points_route_refuses_too_few_rows_and_survives_noise(mh, tmp_path):
    rng = np.random.default_rng(36)
    r, _ = _run(mh, rng.random((7, 4)) * 1000, tmp_path, "seven", ["--points"])
    assert r.returncode == 1 and "Features are not set" in r.stderr
    noise = np.concatenate([rng.random((3000, 2)) * 1000, rng.random((3000, 2)) * 1000], axis=1)
    r, out = _run(mh, noise, tmp_path, "noise", ["--points"])
    assert r.returncode in (0, 1), r.stdout[-2000:] + r.stderr[-2000:]
    if r.returncode == 0:
        res = np.loadtxt(out, ndmin=2)
        assert len(set(int(v) for v in res[:, 4]) - {-1}) <= 2
    else:
        assert "No homographies were found" in r.stderr


def test_harness_3pt_estimator_with_affinities(mh, tmp_path):
    """--estimator 3pt on input WITH affinities: the caller who has them may still choose the point-only refits."""
    sc = mh.synth.make_scene(5000, 3, seed=37, with_neighbours=False)
    rows = np.concatenate([sc.src, sc.dst, sc.aff], axis=1)
    r, out = _run(mh, rows, tmp_path, "aff3", ["--estimator", "3pt"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = np.loadtxt(out, ndmin=2)
    assert res.shape[1] == 9
    assert abs(len(set(int(v) for v in res[:, 8]) - {-1}) - 3) <= 1
