#!/usr/bin/env python3
"""What the symmetric route (mh_set_residual_scope(MH_RESIDUAL_SCOPE_ROUTE) under MH_RESIDUAL_SYMMETRIC, MultiH::SetResidual,
multih_harness --residual symmetric) costs and what it does to the results, next to the forward route, on one MI355X, both in
the same process:

  1. mh_cost_matrix at 50 000 points x 100 000 DLT hypotheses under the route (k_cost_matrix<16, ., true>), beside two
     yardsticks: the forward FP64 k_cost_matrix (mh_set_tuning key 15 = 0) and the symmetric residual sweep
     (mh_residual_matrix under the symmetric mode).  Kernel ms by the engine's events (mh_profile_get), REPEAT launches.
     FP64 instructions per pair as the source states them: d2 57 (two transfers of 28 and one addition; the residual sweep's
     figure), the data term 18 (the IEEE division 11, `1.0 -` 1, `lam *` 1, round() 4, the conversion 1) — 75; the forward
     kernel 28 + 18 = 46.  The share of the FP64 vector issue rate is pairs x instructions / (time x 256 CUs x 64 lanes x 2.4 GHz).
  2. mh_data_cost at 50 000 points x 11 labels and 20 000 x 540, forward against route (kernel ms, mh_profile_get).
  3. mh_inlier_moments at the same two shapes, forward against route (wall time of the call: it has no event of its own).
  4. Process() on synthetic scenes with ground truth (50 000 / 10, 20 000 / 6, 5 000 / 3, seed 1234, the default route with
     2 hypotheses per point) and on the three-moving-planes scene (tests/reestimate_dlt_numpy.py::three_motions, 20 000 points,
     epipolar-free), forward against symmetric, at thr_hom and at thr_hom * sqrt(2): planes recovered, ARI, wall time (median of
     RUNS further calls), RMS distance of the returned models to the truth (each true plane's own points mapped by its best
     returned model, px).
  5. barrsmith (tests/golden/barrsmith.npz), the reference's kept rows, the default route, the twelve seeds of
     profiles/r06_barrsmith_agreement.txt: planes, ARI on the reference's inliers — median, best, worst.

  python tools/symmetric_route_probe.py > profiles/symmetric_route_probe.txt
Env: REPEAT (10), RUNS (5), PARTS ("12345")."""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
mh = importlib.import_module("multi-h_amd")

REPEAT = int(os.environ.get("REPEAT", 10))
RUNS = int(os.environ.get("RUNS", 5))
PARTS = os.environ.get("PARTS", "12345")
SEEDS = (1234, 7, 99, 1, 2, 3, 4, 5, 6, 8, 9, 10)
ISSUE_RATE = 256 * 64 * 2.4e9              # FP64 vector lane-instructions per second
OPS_FORWARD, OPS_SYMMETRIC, OPS_SWEEP_SYM = 46, 75, 57
host = C.CDLL(os.path.join(ROOT, "multi-h_amd", "libmultih_host.so"))
host.mhh_set_residual.argtypes, host.mhh_set_residual.restype = [C.c_int], None
host.mhh_set_epipolar_free.argtypes, host.mhh_set_epipolar_free.restype = [C.c_int], None
dp = C.POINTER(C.c_double)


def kernel_ms(e, key, call):
    call()
    e.synchronize()
    ts = []
    for _ in range(REPEAT):
        e.profile_reset()
        e.profile_enable(True)
        call()
        e.synchronize()
        n, ms = e.profile_get(key)
        e.profile_enable(False)
        ts.append(ms / max(n, 1))
    return ts


def line(name, ts, pairs=None, ops=None):
    tail = ""
    if pairs:
        tail = f"  {ops} FP64 instructions per pair: {pairs * ops / (statistics.median(ts) * 1e-3 * ISSUE_RATE):.2f} of the FP64 vector issue rate at 2.4 GHz"
    print(f"{name:44s}: median of {len(ts)} {statistics.median(ts):9.4f} ms (min {min(ts):.4f}, max {max(ts):.4f}){tail}", flush=True)


def cost_matrix():
    print("== 1. mh_cost_matrix, 50 000 points x 100 000 DLT hypotheses (kernel time, mh_profile_get) ==", flush=True)
    sc = mh.synth.make_scene(50000, 10, seed=1234, with_neighbours=False)
    pairs = 50000 * 100000
    with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
        e.set_correspondences(sc.src, sc.dst, sc.aff)
        e.propose_dlt4(1234, 0, 100000)
        for _ in range(2):
            e.set_residual_mode(False)
            e.set_residual_scope("score")
            e.set_tuning(15, 1)
            line("forward, the FP32 pre-test (default)", kernel_ms(e, mh.capi.K_COSTMATRIX, lambda: e.cost_matrix(fetch_C=False, fetch_counts=False)))
            e.set_tuning(15, 0)
            line("forward, FP64 k_cost_matrix (key 15 = 0)", kernel_ms(e, mh.capi.K_COSTMATRIX, lambda: e.cost_matrix(fetch_C=False, fetch_counts=False)),
                 pairs, OPS_FORWARD)
            e.set_tuning(15, 1)
            e.set_residual_mode(True)
            line("symmetric residual sweep (mh_residual_matrix)", kernel_ms(e, mh.capi.K_RESIDUAL, lambda: e.residual_matrix(2.2 * 2.2, fetch_R=False, fetch_counts=False)),
                 pairs, OPS_SWEEP_SYM)
            e.set_residual_scope("route")
            line("symmetric route, k_cost_matrix<16, ., true>", kernel_ms(e, mh.capi.K_COSTMATRIX, lambda: e.cost_matrix(fetch_C=False, fetch_counts=False)),
                 pairs, OPS_SYMMETRIC)
    print(flush=True)


def shapes():
    for n, labels in ((50000, 11), (20000, 540)):
        sc = mh.synth.make_scene(n, 10, seed=1234, with_neighbours=False)
        m = labels - 1
        H = np.tile(sc.H_true, ((m + 9) // 10, 1))[:m] * (1.0 + np.random.default_rng(0).normal(0, 1e-4, size=(m, 9)))
        yield n, labels, sc, np.ascontiguousarray(H)


def data_cost():
    print("== 2. mh_data_cost (kernel time, mh_profile_get) ==", flush=True)
    for n, labels, sc, H in shapes():
        with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
            e.set_correspondences(sc.src, sc.dst, sc.aff)
            e.set_models(H)
            for name, on in (("forward", False), ("route", True), ("forward", False), ("route", True)):
                e.set_residual_mode(on)
                e.set_residual_scope("route" if on else "score")
                line(f"{n} points x {labels} labels, {name}", kernel_ms(e, mh.capi.K_DATACOST, lambda: e.data_cost(fetch=False)))
    print(flush=True)


def moments():
    print("== 3. mh_inlier_moments (wall time of the call, results fetched) ==", flush=True)
    for n, labels, sc, H in shapes():
        with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
            e.set_correspondences(sc.src, sc.dst, sc.aff)
            e.set_models(H)
            for name, on in (("forward", False), ("route", True), ("forward", False), ("route", True)):
                e.set_residual_mode(on)
                e.set_residual_scope("route" if on else "score")
                e.inlier_moments(2.2 * 2.2)
                ts = []
                for _ in range(3 * REPEAT):
                    t0 = time.perf_counter()
                    e.inlier_moments(2.2 * 2.2)
                    ts.append((time.perf_counter() - t0) * 1e3)
                line(f"{n} points x {labels - 1} models, {name}", ts)
    print(flush=True)


def run_process(sc, thr, hyp, seed=1234, with_F=True):
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((256, 9))
    src, dst, aff = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff))
    F, e2 = (np.ascontiguousarray(sc.F), np.ascontiguousarray(sc.e2)) if with_F else (None, None)
    t0 = time.perf_counter()
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n,
                             F.ctypes.data_as(dp) if with_F else None, e2.ctypes.data_as(dp) if with_F else None, C.c_double(2.6), C.c_double(thr),
                             C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(seed), hyp, 32, 20, None, 0,
                             labels.ctypes.data_as(C.POINTER(C.c_int)), Hout.ctypes.data_as(dp), 256, None, None, None, 0, 4)
    return k, labels, Hout[:max(k, 0)].copy(), (time.perf_counter() - t0) * 1e3


def model_rms(sc, H):
    """RMS over the true planes of the distance, on the plane's own points, between the truth's image and that of the returned
    model that maps them best (px); planes no model comes within 100 px of are counted apart."""
    if len(H) == 0:
        return float("nan"), int(sc.H_true.shape[0])
    sq, lost = [], 0
    for p in range(sc.H_true.shape[0]):
        pts = sc.src[sc.gt_label == p]
        want = mh.synth.apply_h(sc.H_true[p], pts)
        with np.errstate(all="ignore"):
            d = [np.nanmean(((mh.synth.apply_h(h, pts) - want) ** 2).sum(axis=1)) for h in H]
        best = np.nanmin(d) if np.isfinite(d).any() else np.inf
        if best < 100.0 ** 2:
            sq.append(best)
        else:
            lost += 1
    return (float(np.sqrt(np.mean(sq))) if sq else float("nan")), lost


def synthetic():
    print("== 4. Process() on scenes with ground truth (default route, 2 hypotheses per point, post-filter on, at most 20 iterations) ==", flush=True)
    import reestimate_dlt_numpy as D
    scenes = [(f"{n} / {k}", mh.synth.make_scene(n, k, seed=1234, with_neighbours=False), False) for n, k in ((50000, 10), (20000, 6), (5000, 3))]
    scenes.append(("three moving planes, 20 000", D.three_motions(20000), True))
    for what, sc, free in scenes:
        planes = int(sc.H_true.shape[0])
        for thr, thr_name in ((2.2, "thr_hom"), (2.2 * np.sqrt(2.0), "thr_hom * sqrt 2")):
            for residual, name in ((0, "forward"), (1, "symmetric")):
                host.mhh_set_residual(residual)
                host.mhh_set_epipolar_free(1 if free else 0)
                try:
                    k, labels, H, _ = run_process(sc, thr, 2 * sc.n, with_F=not free)
                    times = [run_process(sc, thr, 2 * sc.n, with_F=not free)[3] for _ in range(RUNS)] if k >= 0 else [float("nan")]
                finally:
                    host.mhh_set_residual(-1)
                    host.mhh_set_epipolar_free(0)
                C.CDLL(None).fflush(None)
                if k < 0:
                    print(f"{what:28s} {thr_name:16s} {name:9s}: Process() failed", flush=True)
                    continue
                q = mh.synth.agreement(sc.gt_label, labels)
                rms, lost = model_rms(sc, H)
                print(f"{what:28s} {thr_name:16s} {name:9s}: clusters {k:2d}  planes recovered {q['planes_recovered']:2d}/{planes}  ARI {q['ari']:.4f}  "
                      f"model RMS {rms:.4f} px ({lost} planes without a model)  Process() median of {RUNS} further calls "
                      f"{statistics.median(times):8.2f} ms (min {min(times):.2f})", flush=True)
    print(flush=True)


def barrsmith():
    print("== 5. barrsmith: agreement with the reference's labels (ARI on the reference's inliers), the reference's rows, DLT route ==", flush=True)
    import barrsmith_agreement as BA
    corr, ref, matched, total = BA.kept_correspondences()
    e = mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20)
    e.set_correspondences(corr[:, 0:2], corr[:, 2:4], corr[:, 4:8])
    F, e2, mask, inl = e.estimate_fundamental(1234 ^ 0xf00d, 4000, 2.6)
    e.close()
    print(f"the reference's rows: {matched} of {total} matched to the input, F from them (seed 1234): {int(inl)} inliers at 2.6 px")
    for residual, name in ((0, "forward"), (1, "symmetric")):
        rows = []
        host.mhh_set_residual(residual)
        try:
            for seed in SEEDS:
                k, labels, it, en = BA.run("dlt", corr, F, e2, seed=seed)
                a = BA.agreement(labels, ref) if k > 0 else {"ari_reference_inliers": float("nan"), "ari_all": float("nan")}
                rows.append((int(k), a["ari_reference_inliers"]))
                print(f"{name:9s} seed {seed:5d}: {k} planes, ARI on the reference's inliers {a['ari_reference_inliers']:.3f}, all {a['ari_all']:.3f}", flush=True)
        finally:
            host.mhh_set_residual(-1)
        C.CDLL(None).fflush(None)
        aris = sorted(r[1] for r in rows)
        print(f"   => {name}: planes {[r[0] for r in rows]}, ARI median {statistics.median(aris):.3f} best {aris[-1]:.3f} worst {aris[0]:.3f}", flush=True)
    print(flush=True)


if "1" in PARTS:
    cost_matrix()
if "2" in PARTS:
    data_cost()
if "3" in PARTS:
    moments()
if "4" in PARTS:
    synthetic()
if "5" in PARTS:
    barrsmith()
