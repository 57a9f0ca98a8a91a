"""The route without epipolar geometry (MultiH::SetEpipolarFree, multih_harness --no-epipolar) and MultiH::ESTIMATOR_DLT through
mhh_run_process and the hooks mhh_set_estimator / mhh_set_epipolar_free, on the three-motion scene of
tests/reestimate_dlt_numpy.py (three independently moving planes: no single fundamental matrix describes the pair)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reestimate_dlt_numpy as D
import refit_h_numpy as R

pytestmark = pytest.mark.gpu

THR_H = 2.2
_cache = {}


def _host(mh):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    for fn in (host.mhh_set_estimator, host.mhh_set_epipolar_free):
        fn.argtypes, fn.restype = [C.c_int], None
    host.mhh_set_proposal_source.argtypes, host.mhh_set_proposal_source.restype = [C.c_int, C.c_int, C.c_int], None
    return host


def _restore(host):
    host.mhh_set_estimator(-1)
    host.mhh_set_epipolar_free(0)
    host.mhh_set_proposal_source(0, 16, 1)


def _motions(n):
    if n not in _cache:
        _cache[n] = D.three_motions(n)
    return _cache[n]


def _run_process(host, sc, aff=True, F=None, e2=None, seed=5, hypotheses=4000, max_models=16, iter_max_new=4):
    dp = C.POINTER(C.c_double)
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((64, 9))
    it, en = C.c_int(-1), C.c_double(-1)
    src, dst, a = (np.ascontiguousarray(v) for v in (sc.src, sc.dst, sc.aff))
    Fp = None if F is None else np.ascontiguousarray(F).ctypes.data_as(dp)
    ep = None if e2 is None else np.ascontiguousarray(e2).ctypes.data_as(dp)
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), a.ctypes.data_as(dp) if aff else None, sc.n, Fp, ep,
                             C.c_double(2.6), C.c_double(THR_H), C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(seed),
                             hypotheses, max_models, 0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 64, C.byref(it), C.byref(en), None, 0, iter_max_new)
    C.CDLL(None).fflush(None)
    return k, labels, Hout[:max(k, 0)].copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_three_motions_are_recovered_without_epipolar_geometry(mh, engine_lib, capfd):
    host = _host(mh)
    sc = _motions(1200)
    try:
        host.mhh_set_epipolar_free(1)
        k, labels, H = _run_process(host, sc)                               # F passed as NULL
        log = capfd.readouterr().out
        stages = (C.c_int * 4)()
        host.mhh_get_front_stages(stages)
        again = _run_process(host, sc)
        points_only = _run_process(host, sc, aff=False)
    finally:
        _restore(host)
    got = mh.synth.agreement(sc.gt_label, labels)
    with capfd.disabled():
        print(f"epipolar-free, 1200 points: {k} models, planes {got['planes_recovered']} of {got['planes']}, ARI {got['ari']:.4f}")
    assert k >= 3 and labels.size == sc.n and labels.min() >= -1 and labels.max() < k
    assert list(stages) == [sc.n] * 4
    assert "compatibility check is skipped" in log
    assert got["planes_recovered"] == 3, got
    for m in range(k):                                                      # every model fits the points labelled with it
        own = labels == m
        assert own.any(), m
        rms = float(np.sqrt(R.d2_of(sc.src[own], sc.dst[own], H[m]).mean()))
        assert rms < THR_H, (m, rms)
    # the same call twice: the same labels and H bit for bit
    assert again[0] == k and np.array_equal(again[1], labels) and np.array_equal(_bits(again[2]), _bits(H))
    # point-only: the affinities are never read
    assert points_only[0] == k and np.array_equal(points_only[1], labels) and np.array_equal(_bits(points_only[2]), _bits(H))


def test_a_given_epipolar_geometry_is_ignored(mh, engine_lib, capfd):
    host = _host(mh)
    sc = _motions(1200)
    F = np.array([0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0])
    try:
        host.mhh_set_epipolar_free(1)
        plain = _run_process(host, sc)
        capfd.readouterr()
        given = _run_process(host, sc, F=F, e2=np.array([1e9, 0.0]))
        log = capfd.readouterr().out
    finally:
        _restore(host)
    assert log.count("SetEpipolarGeometry is ignored") == 1
    assert given[0] == plain[0] and np.array_equal(given[1], plain[1]) and np.array_equal(_bits(given[2]), _bits(plain[2]))


@pytest.mark.parametrize("what", ["stable_sets", "haf_proposals", "3pt_proposals"])
def test_what_needs_the_fundamental_matrix_is_refused(mh, engine_lib, capfd, what):
    host = _host(mh)
    sc = _motions(1200)
    try:
        host.mhh_set_epipolar_free(1)
        if what == "haf_proposals":
            host.mhh_set_proposal_source(1, 16, 1)
        elif what == "3pt_proposals":
            host.mhh_set_proposal_source(2, 0, 1)
        capfd.readouterr()
        k = _run_process(host, sc, iter_max_new=-1 if what == "stable_sets" else 4)[0]
        err = capfd.readouterr().err
    finally:
        _restore(host)
    assert k == -1
    assert "need the fundamental matrix" in err and "epipolar-free route" in err
    assert {"stable_sets": "INIT_STABLE_SETS", "haf_proposals": "PROPOSAL_SOURCE_HAF", "3pt_proposals": "PROPOSAL_SOURCE_3PT"}[what] in err


def test_the_default_route_is_what_it_was(mh, engine_lib):
    """With mhh_set_estimator(-1) and mhh_set_epipolar_free(0) — the statics' initial values, which every test of this file
    restores — the default route gives the same labels and H before and after the switches have been on in between."""
    host = _host(mh)
    sc = mh.synth.make_scene(1500, 3, seed=17, with_neighbours=False)
    before = _run_process(host, sc, F=sc.F, e2=sc.e2)                       # both hooks at their initial values, -1 and 0
    try:
        host.mhh_set_epipolar_free(1)
        _run_process(host, sc)
        host.mhh_set_epipolar_free(0)
        host.mhh_set_estimator(2)
        with_dlt = _run_process(host, sc, F=sc.F, e2=sc.e2)                 # the DLT refits on the route WITH F
    finally:
        _restore(host)
    after = _run_process(host, sc, F=sc.F, e2=sc.e2)
    assert before[0] >= 2
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(_bits(after[2]), _bits(before[2]))
    assert with_dlt[0] >= 2 and with_dlt[1].min() >= -1 and with_dlt[1].max() < with_dlt[0]


def test_harness_switches(mh, engine_lib, tmp_path):
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    sc = _motions(1200)
    runs = (("points", np.concatenate([sc.src, sc.dst], axis=1), ["--points", "--no-epipolar"], 4),
            ("affine", np.concatenate([sc.src, sc.dst, sc.aff], axis=1), ["--no-epipolar", "--estimator", "dlt"], 8))
    for name, rows, extra, cols in runs:
        corr, out = tmp_path / f"{name}.txt", tmp_path / f"{name}.out"
        np.savetxt(corr, rows, fmt="%.17g")
        r = subprocess.run([harness, str(corr), str(out), *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        res = np.loadtxt(out, ndmin=2)
        assert res.shape == (sc.n, cols + 1)                                # no row is dropped; the last column is the label
        found = set(int(v) for v in res[:, cols]) - {-1}
        assert len(found) >= 2, found
    # --estimator dlt alone: the route with F, whose refits are then DLT fits
    sc2 = mh.synth.make_scene(3000, 3, seed=37, with_neighbours=False)
    corr, out = tmp_path / "dlt.txt", tmp_path / "dlt.out"
    np.savetxt(corr, np.concatenate([sc2.src, sc2.dst, sc2.aff], axis=1), fmt="%.17g")
    r = subprocess.run([harness, str(corr), str(out), "--estimator", "dlt"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = np.loadtxt(out, ndmin=2)
    assert res.shape[1] == 9 and len(set(int(v) for v in res[:, 8]) - {-1}) >= 2
