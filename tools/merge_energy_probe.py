#!/usr/bin/env python3
"""What the energy-tested merge (mh_merge_deltas, mh_labeling_energy; MultiH::SetMergeMode(MERGE_ENERGY), multih_harness --merge
energy) costs and what it does to the results, next to the default mean-shift merge, on one MI355X, both in the same process:

  1. mh_merge_deltas at 50 000 points / 11 labels / 55 pairs and at 20 000 points / 540 labels / each label's 8 nearest labels
     in the 6-D feature space (the pair list of the MergingStep: mhh_merge_pair_list), mh_labeling_energy at both sizes, and
     beside them mh_reestimate under "dlt" on the same labels — the yardstick for "a pair costs about a label's fit".  Wall time
     around call + mh_synchronize, 3 warm-up calls, median and spread of 20 calls.
  2. Process() on the flagship scenes with ground truth (50 000 / 10, 20 000 / 6, 5 000 / 3, seed 1234, 2 hypotheses per point)
     and on the three-moving-planes scene (tests/reestimate_dlt_numpy.py::three_motions, 20 000 points, epipolar-free), the
     default merge against MERGE_ENERGY: the second call of the process is timed; clusters, planes recovered, ARI, and the merge
     log's totals.
  3. barrsmith (tests/golden/barrsmith.npz) from the raw file over the twelve seeds of tools/barrsmith_agreement.py, both modes:
     clusters, the reference's planes recovered and ARI on the reference's inliers (median, min, max), the merge log's totals.

  python tools/merge_energy_probe.py > profiles/merge_energy_probe.txt
Env: PARTS ("123")."""
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

PARTS = os.environ.get("PARTS", "123")
WARMUP, CALLS = 3, 20
SEEDS = (1234, 7, 99, 1, 2, 3, 4, 5, 6, 8, 9, 10)
host = C.CDLL(os.path.join(ROOT, "multi-h_amd", "libmultih_host.so"))
host.mhh_set_merge_mode.argtypes, host.mhh_set_merge_mode.restype = [C.c_int], None
host.mhh_set_epipolar_free.argtypes, host.mhh_set_epipolar_free.restype = [C.c_int], None
dp = C.POINTER(C.c_double)


def wall_ms(e, call):
    for _ in range(WARMUP):
        call()
        e.synchronize()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()
        e.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def line(name, ts):
    print(f"{name:58s}: median of {len(ts)} {statistics.median(ts):9.4f} ms (min {min(ts):.4f}, max {max(ts):.4f})", flush=True)


def pair_list(H):
    nh = H.shape[0]
    out = np.zeros((nh * max(nh - 1, 8), 2), dtype=np.int32)
    k = host.mhh_merge_pair_list(np.ascontiguousarray(H).ctypes.data_as(dp), nh, 64, 8, out.ctypes.data_as(C.POINTER(C.c_int)))
    return np.ascontiguousarray(out[:k])


def merge_log():
    log = np.zeros((512, 9), dtype=np.int64)
    k = host.mhh_get_merge_log(log.ctypes.data_as(C.POINTER(C.c_longlong)), 512)
    log = log[:min(k, 512)]
    return (f"{len(log)} steps, {int(log[:, 2].sum())} pairs, {int(log[:, 3].sum())} joined, {int(log[:, 4].sum())} filtered, "
            f"sum of deltas {int(log[:, 6].sum())}") if len(log) else "no step evaluated"


def timings():
    print(f"== 1. wall time of call + mh_synchronize, {WARMUP} warm-up calls, {CALLS} timed ==", flush=True)
    for n, m in ((50000, 11), (20000, 540)):
        sc = mh.synth.make_scene(n, 10, seed=1234, with_neighbours=False)
        rng = np.random.default_rng(0)
        H = np.ascontiguousarray(np.tile(sc.H_true, ((m + 9) // 10, 1))[:m] * (1.0 + rng.normal(0, 1e-4, size=(m, 9))))
        lab = np.where(sc.gt_label >= 0, sc.gt_label + 10 * rng.integers(0, (m + 9) // 10, size=n), -1)
        lab = np.where(lab < m, lab, -1).astype(np.int32)
        with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
            e.set_correspondences(sc.src, sc.dst, sc.aff)
            e.build_neighbors_knn(16)
            e.set_estimator("dlt")
            e.set_models(H)
            pairs = pair_list(H)
            _, _, _, status = e.merge_deltas(lab, pairs)
            what = f"{n} points / {m} models"
            line(f"{what}, mh_merge_deltas, {len(pairs)} pairs ({int((status == 0).sum())} OK)", wall_ms(e, lambda: e.merge_deltas(lab, pairs)))
            line(f"{what}, mh_labeling_energy", wall_ms(e, lambda: e.labeling_energy(lab)))
            ts = []
            for i in range(WARMUP + CALLS):                   # the fit replaces the models: set them again, outside the clock
                e.set_models(H)
                e.synchronize()
                t0 = time.perf_counter()
                e.reestimate(lab)
                e.synchronize()
                if i >= WARMUP:
                    ts.append((time.perf_counter() - t0) * 1e3)
            line(f"{what}, mh_reestimate under \"dlt\" ({m} fits)", ts)
    print(flush=True)


def run_process(sc, hyp, seed=1234, with_F=True):
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((256, 9))
    src, dst, aff = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff))
    F, e2 = (np.ascontiguousarray(sc.F), np.ascontiguousarray(sc.e2)) if with_F else (None, None)
    t0 = time.perf_counter()
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n,
                             F.ctypes.data_as(dp) if with_F else None, e2.ctypes.data_as(dp) if with_F else None, C.c_double(2.6), C.c_double(2.2),
                             C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(seed), hyp, 32, 20, None, 0,
                             labels.ctypes.data_as(C.POINTER(C.c_int)), Hout.ctypes.data_as(dp), 256, None, None, None, 0, 4)
    return k, labels, (time.perf_counter() - t0) * 1e3


def synthetic():
    print("== 2. Process() on scenes with ground truth (2 hypotheses per point, post-filter on, at most 20 iterations; the second call is timed) ==", flush=True)
    import reestimate_dlt_numpy as D
    scenes = [(f"{n} / {k}", mh.synth.make_scene(n, k, seed=1234, with_neighbours=False), False) for n, k in ((50000, 10), (20000, 6), (5000, 3))]
    scenes.append(("three moving planes, 20 000", D.three_motions(20000), True))
    for what, sc, free in scenes:
        planes = int(sc.H_true.shape[0])
        for mode, name in ((0, "meanshift"), (1, "energy")):
            host.mhh_set_merge_mode(mode)
            host.mhh_set_epipolar_free(1 if free else 0)
            try:
                run_process(sc, 2 * sc.n, with_F=not free)
                k, labels, ms = run_process(sc, 2 * sc.n, with_F=not free)
                log = merge_log()
            finally:
                host.mhh_set_merge_mode(-1)
                host.mhh_set_epipolar_free(0)
            C.CDLL(None).fflush(None)
            if k < 0:
                print(f"{what:28s} {name:9s}: Process() failed", flush=True)
                continue
            q = mh.synth.agreement(sc.gt_label, labels)
            print(f"{what:28s} {name:9s}: clusters {k:2d}  planes recovered {q['planes_recovered']:2d}/{planes}  ARI {q['ari']:.4f}  "
                  f"Process() {ms:8.2f} ms  merge log: {log}", flush=True)
    print(flush=True)


def barrsmith():
    print("== 3. barrsmith from the raw file (load filter 2 px, point-to-line distance, DLT route), compared on the rows both kept ==", flush=True)
    import barrsmith_agreement as BA
    pts, ref_rows, ref_labels = BA.kept_correspondences(with_rows=True)
    for mode, name in ((0, "meanshift"), (1, "energy")):
        rows_out = []
        host.mhh_set_merge_mode(mode)
        try:
            for seed in SEEDS:
                rows, labels, k, _ = BA.harness_route(pts, "dlt", seed)
                log = merge_log()
                full = np.full(len(pts), -2, dtype=int)
                full[rows] = labels
                ours = full[ref_rows]
                both = ours > -2
                ari = BA.agreement(ours[both], ref_labels[both])["ari_reference_inliers"] if k > 0 else float("nan")
                # the reference's planes recovered: one of our labels holds >= 80 % of the plane's rows, no label counted twice
                planes = mh.synth.agreement(ref_labels[both], ours[both])["planes_recovered"] if k > 0 else 0
                rows_out.append((int(k), ari, int(planes)))
                print(f"{name:9s} seed {seed:5d}: {k} clusters, {planes}/5 of the reference's planes recovered, ARI on the reference's inliers {ari:.3f}; "
                      f"merge log: {log}", flush=True)
        finally:
            host.mhh_set_merge_mode(-1)
        C.CDLL(None).fflush(None)
        aris = sorted(r[1] for r in rows_out)
        ks = sorted(r[0] for r in rows_out)
        ps = sorted(r[2] for r in rows_out)
        print(f"   => {name}: clusters {[r[0] for r in rows_out]} (median {statistics.median(ks)}, min {ks[0]}, max {ks[-1]}; the reference has 5 planes), "
              f"planes recovered {[r[2] for r in rows_out]} (median {statistics.median(ps)}, min {ps[0]}, max {ps[-1]}), "
              f"ARI median {statistics.median(aris):.3f} min {aris[0]:.3f} max {aris[-1]:.3f}", flush=True)
    print(flush=True)


if "1" in PARTS:
    timings()
if "2" in PARTS:
    synthetic()
if "3" in PARTS:
    barrsmith()
