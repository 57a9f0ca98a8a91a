"""GPU tests of the compatibility check without F: mh_compat_dlt_medians (csrc/dlt4.hip k_dlt4 under the segment sampler,
csrc/compat.hip k_compat_median4 and k_compat_cluster_median) against its twin tests/compat_dlt_numpy.py — tuples, fits, trial
values and cluster medians bit for bit —, its errors, that it leaves the engine's state alone, multih::CompatibilityCheckDlt on
the engine (mhh_compatibility_dlt_on_engine) and the route through MultiH::SetCompatibilityFit (mhh_set_compat_fit)."""
import ctypes as C
import os

import numpy as np
import pytest

import compat_dlt_numpy as T
import reestimate_dlt_numpy as D

pytestmark = pytest.mark.gpu
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
THR_H = 2.2
FIT_3PT, FIT_DLT = 0, 1
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _points(synth, sizes, seed=17):
    total = int(sum(sizes))
    sc = synth.make_scene(max(total, 2000), 3, seed=seed, noise=0.6, outlier_frac=0.3, with_neighbours=False)
    pts = np.concatenate([sc.src, sc.dst], axis=1)[:total].copy()
    begin = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return pts, begin


# ---- 1. tuples and fits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,trials", [((5, 6, 19, 64, 257), 7), ((5003, 20), 65)])
@pytest.mark.parametrize("first", [0, 2 ** 33 + 3])
def test_tuples_and_fits_are_the_twins(engine, synth, oracle, sizes, trials, first):
    """35 hypotheses: several clusters share one wavefront's 16 and the last wave is partly dead; 130: past the 64 hypotheses of
    a workgroup.  The tuples are sample4's per cluster, shifted by the cluster's start; the fits are oracle.dlt4's on them."""
    pts, begin = _points(synth, sizes)
    med, val, H, idx = engine.compat_dlt_medians(pts, begin, 99, first, trials)
    want = T.tuples(99, first, trials, sizes)
    for c in range(len(sizes)):
        assert np.array_equal(idx[c], want[c] + begin[c]), c
        assert idx[c].min() >= begin[c] and idx[c].max() < begin[c + 1]
    with np.errstate(all="ignore"):
        H_ref, wit, _ = oracle.dlt4(pts[:, :2], pts[:, 2:], idx.reshape(-1, 4))
    good = wit > 1e-6
    print(f"witness > 1e-6 on {int(good.sum())} of {good.size} trials")
    assert good.sum() > 0.5 * good.size
    assert np.array_equal(_bits(H.reshape(-1, 9)[good]), _bits(H_ref[good]))


# ---- 2. trial values ----------------------------------------------------------------------------------------------------
def _trial_cases(synth):
    sizes = (257, 1000, 5003, 5, 40, 31)
    pts, begin = _points(synth, sizes, seed=19)
    b = begin
    pts[b[4] + 5:b[4] + 30] = pts[b[4] + 5]              # 25 of 40 members are one point: the rank falls into a run of equal keys
    pts[b[5]:b[6]] = pts[b[5]]                           # one point throughout: no fit is finite
    return sizes, pts, begin


def test_trial_values_are_the_sorted_keys_under_the_engines_fits(engine, synth):
    sizes, pts, begin = _trial_cases(synth)
    trials = 9
    med, val, H, idx = engine.compat_dlt_medians(pts, begin, 5, 0, trials)
    w_med, w_val, _, w_idx, _ = T.medians(pts, begin, 5, 0, trials, H=H)
    assert np.array_equal(idx, w_idx)
    assert np.array_equal(_bits(val), _bits(w_val))
    assert np.array_equal(_bits(med), _bits(w_med))
    # the cases are what they claim to be
    assert not np.isfinite(H[5]).all(axis=1).any() and np.isposinf(val[5]).all() and np.isposinf(med[5])
    assert np.isfinite(val[:4]).all()
    rep = begin[4] + 5                                   # 21 or more of the at most 36 others are this point: the rank is in its run
    for t in range(trials):
        with np.errstate(all="ignore"):
            d = T.O.residual_matrix(pts[rep:rep + 1, :2], pts[rep:rep + 1, 2:], H[4, t:t + 1])[0, 0]
        assert _bits(val[4, t]) == _bits(np.inf if np.isnan(d) else d)     # (a tuple that draws the point twice fits nothing finite)
    for t in range(trials):                              # nc = 5: the one member that is not in the tuple
        left = np.setdiff1d(np.arange(begin[3], begin[4]), idx[3, t])
        assert left.size == 1
        d = T.O.residual_matrix(pts[left, :2], pts[left, 2:], H[3, t:t + 1])[0, 0]
        assert _bits(val[3, t]) == _bits(d)


# ---- 3. cluster medians -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trials", [1, 2, 7, 501])
def test_cluster_median_is_the_lower_median_of_the_engines_trial_values(engine, synth, trials):
    pts, begin = _points(synth, (64, 300, 5))
    med, val, _, _ = engine.compat_dlt_medians(pts, begin, 11, 3, trials)
    assert np.array_equal(_bits(med), _bits(np.sort(val, axis=1)[:, (trials - 1) // 2]))


# ---- 4. errors ----------------------------------------------------------------------------------------------------------
def test_error_codes(mh, engine):
    lib, h = engine.lib, engine._h
    pts = np.random.default_rng(0).uniform(0, 100, size=(5200, 4))
    med = np.empty(2048)
    pp, mp = pts.ctypes.data_as(_dp), med.ctypes.data_as(_dp)

    def call(e=h, p=pp, begin=(0, 6, 12), clusters=None, first=0, trials=3, m=mp):
        b = None if begin is None else np.asarray(begin, dtype=np.int32)
        return lib.mh_compat_dlt_medians(e, p, None if b is None else b.ctypes.data_as(_ip), b.size - 1 if clusters is None else clusters,
                                         C.c_ulonglong(1), C.c_longlong(first), trials, m, None, None, None)

    many = np.arange(0, 5 * 1026, 5)                                        # 1025 clusters of 5 points
    bad = [dict(e=None), dict(p=None), dict(begin=None, clusters=2), dict(m=None), dict(clusters=0), dict(clusters=-1),
           dict(begin=(1, 7, 13)), dict(begin=(0, 12, 6)), dict(begin=(0, 6, 10)), dict(begin=(0, 4)), dict(trials=0),
           dict(trials=4097), dict(first=-1), dict(begin=many, trials=4096)]
    for kw in bad:
        assert call(**kw) == -2, kw
        assert call() == 0, kw                                             # a valid call right behind it
    assert call(begin=many[:1025], trials=4096) == 0                       # 1024 x 4096 = 2^22 trials is the limit itself
    with pytest.raises(mh.MultiHError):
        engine.compat_dlt_medians(pts[:8], [0, 4, 8], 1, 0, 3)


# ---- 5. state untouched -------------------------------------------------------------------------------------------------
def test_engine_state_is_untouched(engine, synth):
    sc = synth.make_scene(1500, 3, seed=4, with_neighbours=False)
    engine.set_correspondences(sc.src, sc.dst)
    pts, begin = _points(synth, (300, 40, 7))
    thr2 = THR_H ** 2

    def run(with_calls):
        call = (lambda: engine.compat_dlt_medians(pts, begin, 8, 0, 33)) if with_calls else (lambda: None)
        engine.propose_dlt4(77, 0, 600)
        call()
        counts = engine.score(thr2)
        call()
        state = (engine.model_count, engine.get_models(), engine.get_samples(), counts, engine.select_best())
        engine.prefetch_dlt4(78, 600, 200)
        call()
        engine.adopt_prefetched()
        return state + (engine.model_count, engine.get_models(), engine.get_samples(), engine.score(thr2))

    plain, mixed = run(False), run(True)
    for a, b in zip(plain, mixed):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert plain[5] == 200 and np.array_equal(plain[7], T.O.sample4(78, 600, 200, sc.n))


# ---- 8. determinism -----------------------------------------------------------------------------------------------------
def test_two_calls_and_two_engines_give_the_same_bits(mh, engine, synth):
    sizes, pts, begin = _trial_cases(synth)
    a = engine.compat_dlt_medians(pts, begin, 5, 17, 40)
    b = engine.compat_dlt_medians(pts, begin, 5, 17, 40)
    with mh.Engine(device=0, thr_fund_mat=2.6, thr_hom=2.2, locality=0.005, lam=0.5, min_inliers=20) as other:
        c = other.compat_dlt_medians(pts, begin, 5, 17, 40)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()


# ---- 6. the host rule on the engine -------------------------------------------------------------------------------------
def _host(mh):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_compat_fit.argtypes, host.mhh_set_compat_fit.restype = [C.c_int, C.c_int, C.c_double], None
    host.mhh_set_epipolar_free.argtypes, host.mhh_set_epipolar_free.restype = [C.c_int], None
    host.mhh_set_post_filter.argtypes, host.mhh_set_post_filter.restype = [C.c_int], None
    return host


def _restore(host):
    host.mhh_set_compat_fit(FIT_3PT, 501, 0.0)
    host.mhh_set_epipolar_free(0)
    host.mhh_set_post_filter(1)


@pytest.mark.parametrize("sizes,min_inliers", [((700, 523, 64, 17), 20), ((40, 33, 5, 4), 0)])
def test_check_on_the_engine_equals_the_twin(mh, engine, synth, sizes, min_inliers):
    host = _host(mh)
    planes, trials, seed = len(sizes), 501, 4242
    limit = T.LIMIT_SCALE * THR_H ** 2
    sc = synth.make_scene(12000, planes, seed=11 + planes, noise=0.4, outlier_frac=0.0, with_neighbours=False)
    labels = np.full(sc.n, -1, dtype=np.int32)
    for c, sz in enumerate(sizes):
        members = np.flatnonzero(sc.gt_label == c)[:sz]
        assert members.size == sz
        labels[members] = c
    scr = np.flatnonzero(labels == 1)
    sc.dst[scr[::2]] = np.random.default_rng(5).uniform(0, 1000, size=(scr[::2].size, 2))      # cluster 1: half scrambled
    src, dst = np.ascontiguousarray(sc.src), np.ascontiguousarray(sc.dst)
    H = sc.H_true.copy(); lab = labels.copy(); med = np.zeros(planes)
    kept = host.mhh_compatibility_dlt_on_engine(engine._h, src.ctypes.data_as(_dp), dst.ctypes.data_as(_dp), sc.n, lab.ctypes.data_as(_ip),
                                                H.ctypes.data_as(_dp), planes, C.c_double(limit), min_inliers, C.c_ulonglong(seed), trials,
                                                med.ctypes.data_as(_dp))
    wits = []

    def medians_of(p, b, s, f, t):
        got = T.medians(p, b, s, f, t)
        wits.append((got[4] > 1e-6).all(axis=1))
        return got[0]
    w_lab, w_H, w_med, w_removed = T.check(src, dst, labels, sc.H_true, limit, min_inliers, seed, trials, medians_of)
    print(f"medians {med}, the twin's {w_med}, removed {w_removed}")
    assert kept == w_H.shape[0] and np.array_equal(lab, w_lab) and np.array_equal(_bits(H[:kept]), _bits(w_H))
    stat = np.flatnonzero(~np.isnan(w_med))
    assert np.array_equal(np.isnan(med), np.isnan(w_med)) and stat.size == wits[0].size
    for q, c in enumerate(stat):
        if wits[0][q]:
            assert _bits(med[c]) == _bits(w_med[c]), c
        else:
            assert abs(med[c] - w_med[c]) <= 1e-6 * w_med[c], c
    want = [False, True, False, True] if min_inliers == 20 else [False, True, False, False]     # (17 members < 20 go by size)
    assert w_removed.tolist() == want
    assert np.isnan(w_med[3]) and np.isfinite(w_med[:3]).all()


# ---- 7. the route -------------------------------------------------------------------------------------------------------
def _run_process(host, sc, F=None, e2=None, seed=5):
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((64, 9))
    it, en = C.c_int(-1), C.c_double(-1)
    src, dst, a = (np.ascontiguousarray(v) for v in (sc.src, sc.dst, sc.aff))
    Fp = None if F is None else np.ascontiguousarray(F).ctypes.data_as(_dp)
    ep = None if e2 is None else np.ascontiguousarray(e2).ctypes.data_as(_dp)
    k = host.mhh_run_process(src.ctypes.data_as(_dp), dst.ctypes.data_as(_dp), a.ctypes.data_as(_dp), sc.n, Fp, ep,
                             C.c_double(2.6), C.c_double(THR_H), C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(seed),
                             4000, 16, 0, None, 0, labels.ctypes.data_as(_ip), Hout.ctypes.data_as(_dp), 64, C.byref(it), C.byref(en),
                             None, 0, 4)
    C.CDLL(None).fflush(None)
    return k, labels, Hout[:max(k, 0)].copy()


def _through_the_twin(sc, raw, seed=5):
    """What Process() returns under COMPAT_FIT_DLT, from its result with the post-filter off (more than one cluster left)."""
    k, labels, H = raw
    lab, Hk, med, removed = T.check(sc.src, sc.dst, labels, H, T.LIMIT_SCALE * THR_H ** 2, 20, seed ^ 0xc0117a7, 501)
    return Hk.shape[0], lab, Hk, removed


def test_the_route_without_epipolar_geometry_runs_the_check(mh, engine_lib, capfd):
    host = _host(mh)
    if "motions" not in _cache:
        _cache["motions"] = D.three_motions(1200)
    sc = _cache["motions"]
    try:
        host.mhh_set_epipolar_free(1)
        host.mhh_set_post_filter(0)
        raw = _run_process(host, sc)
        host.mhh_set_post_filter(1)
        capfd.readouterr()
        plain = _run_process(host, sc)                                      # the hook at its initial value: the parent's behaviour
        log_plain = capfd.readouterr().out
        host.mhh_set_compat_fit(FIT_DLT, 501, 0.0)
        got = _run_process(host, sc)
        log = capfd.readouterr().out
        host.mhh_set_compat_fit(FIT_DLT, 501, 0.01)                         # a limit no noisy plane passes: limit_scale arrives
        capfd.readouterr()
        _run_process(host, sc)
        log_strict = capfd.readouterr().out
        host.mhh_set_post_filter(0)
        off = _run_process(host, sc)                                        # SetCompatibilityCheck(false) still switches it off
    finally:
        _restore(host)
    assert "compatibility check is skipped" in log_plain and "4-point trials" not in log_plain
    assert plain[0] == raw[0] and np.array_equal(plain[1], raw[1]) and np.array_equal(_bits(plain[2]), _bits(raw[2]))
    assert off[0] == raw[0] and np.array_equal(off[1], raw[1]) and np.array_equal(_bits(off[2]), _bits(raw[2]))
    assert "Compatibility check (4-point trials)" in log and "clusters removed" in log and "is skipped" not in log
    strict = T.check(sc.src, sc.dst, raw[1], raw[2], 0.01 * THR_H ** 2, 20, 5 ^ 0xc0117a7, 501)
    assert strict[3].all() and f"({raw[0]} clusters removed from {raw[0]})" in log_strict
    want = _through_the_twin(sc, raw)
    with capfd.disabled():
        print(f"epipolar-free with the 4-point check: {raw[0]} clusters in, {got[0]} out (the twin removes {want[3]})")
    assert raw[0] > 1 and want[0] > 1
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2]))
    agreement = mh.synth.agreement(sc.gt_label, got[1])
    assert agreement["planes_recovered"] == 3, agreement


def test_the_default_route_runs_the_check_when_asked(mh, engine_lib, capfd):
    host = _host(mh)
    sc = mh.synth.make_scene(1500, 3, seed=17, with_neighbours=False)
    try:
        host.mhh_set_post_filter(0)
        raw = _run_process(host, sc, F=sc.F, e2=sc.e2)
        host.mhh_set_post_filter(1)
        host.mhh_set_compat_fit(FIT_DLT, 501, 0.0)
        capfd.readouterr()
        got = _run_process(host, sc, F=sc.F, e2=sc.e2)
        log = capfd.readouterr().out
    finally:
        _restore(host)
    assert "Compatibility check (4-point trials)" in log
    want = _through_the_twin(sc, raw)
    assert raw[0] > 1 and want[0] > 1
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2]))


def test_the_harness_flag_runs_the_check(mh, engine_lib, tmp_path):
    import subprocess
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    if "motions" not in _cache:
        _cache["motions"] = D.three_motions(1200)
    sc = _cache["motions"]
    corr, out = tmp_path / "points.txt", tmp_path / "points.out"
    np.savetxt(corr, np.concatenate([sc.src, sc.dst], axis=1), fmt="%.17g")
    r = subprocess.run([harness, str(corr), str(out), "--points", "--no-epipolar", "--compat-fit", "dlt:101:256"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Compatibility check (4-point trials)" in r.stdout and "clusters removed" in r.stdout and "is skipped" not in r.stdout
    res = np.loadtxt(out, ndmin=2)
    assert res.shape == (sc.n, 5) and len(set(int(v) for v in res[:, 4]) - {-1}) >= 2
