#!/usr/bin/env python3
"""What the label cost of the energy-tested merge (mh_best_alternative, mh_drop_deltas; MultiH::SetLabelCost, multih_harness
--label-cost) costs and what it does to the results, on one MI355X, everything in the same process:

  1. mh_best_alternative and mh_drop_deltas (every label a candidate) at 50 000 points / 11 labels and at 20 000 points / 540
     labels, beside mh_merge_deltas (the MergingStep's pair list) and mh_data_cost (the N x Nh table the arg-min never writes;
     on the device, not fetched) at the same sizes.  Wall time around call + mh_synchronize, 3 warm-up calls, median and spread
     of 20 calls.
  2. Process() under MERGE_ENERGY on the three synthetic flagship scenes (50 000 / 10, 20 000 / 6, 5 000 / 3, seed 1234, 2
     hypotheses per point), label cost 0 against a positive one: the second call of the process is timed; clusters, planes
     recovered, ARI, and the totals of the merge and drop logs.
  3. barrsmith (tests/golden/barrsmith.npz) from the raw file over the twelve seeds of tools/barrsmith_agreement.py, DLT route,
     MERGE_ENERGY, label cost 0, 10, 20, 40: clusters, the reference's planes recovered and ARI on the reference's inliers
     (median, min, max), joins and drops per run.

  python tools/label_cost_probe.py > profiles/label_cost_probe.txt
Env: PARTS ("123"), COST (the positive cost of part 2, default 40)."""
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ["PARTS"], PARTS = "", os.environ.get("PARTS", "123")      # the merge probe's helpers without its own run
import merge_energy_probe as P

mh, host = P.mh, P.host
host.mhh_set_label_cost.argtypes, host.mhh_set_label_cost.restype = [C.c_double], None
COST = float(os.environ.get("COST", "40"))


def drop_log():
    log = np.zeros((512, 9), dtype=np.int64)
    k = host.mhh_get_drop_log(log.ctypes.data_as(C.POINTER(C.c_longlong)), 512)
    log = log[:min(k, 512)]
    hit = log[log[:, 2] >= 0] if len(log) else log
    return len(log), len(hit), int(hit[:, 3].sum()) if len(hit) else 0, int(hit[:, 4].sum()) if len(hit) else 0


def joins():
    log = np.zeros((512, 9), dtype=np.int64)
    k = host.mhh_get_merge_log(log.ctypes.data_as(C.POINTER(C.c_longlong)), 512)
    return int(log[:min(k, 512), 3].sum())


def timings():
    print(f"== 1. wall time of call + mh_synchronize, {P.WARMUP} warm-up calls, {P.CALLS} timed ==", flush=True)
    for n, m in ((50000, 11), (20000, 540)):
        sc = mh.synth.make_scene(n, 10, seed=1234, with_neighbours=False)
        rng = np.random.default_rng(0)
        H = np.ascontiguousarray(np.tile(sc.H_true, ((m + 9) // 10, 1))[:m] * (1.0 + rng.normal(0, 1e-4, size=(m, 9))))
        lab = np.where(sc.gt_label >= 0, sc.gt_label + 10 * rng.integers(0, (m + 9) // 10, size=n), -1)
        lab = np.where(lab < m, lab, -1).astype(np.int32)
        cand = np.arange(m, dtype=np.int32)
        with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
            e.set_correspondences(sc.src, sc.dst, sc.aff)
            e.build_neighbors_knn(16)
            e.set_models(H)
            pairs = P.pair_list(H)
            status = e.drop_deltas(lab, cand)[2]
            what = f"{n} points / {m} models"
            P.line(f"{what}, mh_best_alternative", P.wall_ms(e, lambda: e.best_alternative(lab)))
            P.line(f"{what}, mh_drop_deltas, {m} candidates ({int((status == 0).sum())} OK)", P.wall_ms(e, lambda: e.drop_deltas(lab, cand)))
            P.line(f"{what}, mh_merge_deltas, {len(pairs)} pairs", P.wall_ms(e, lambda: e.merge_deltas(lab, pairs)))
            P.line(f"{what}, mh_data_cost (table left on the device)", P.wall_ms(e, lambda: e.data_cost(fetch=False)))
    print(flush=True)


def synthetic():
    print("== 2. Process() under MERGE_ENERGY on the flagship scenes (2 hypotheses per point, post-filter on, at most 20 iterations; the second call is timed) ==", flush=True)
    for n, k_true in ((50000, 10), (20000, 6), (5000, 3)):
        sc = mh.synth.make_scene(n, k_true, seed=1234, with_neighbours=False)
        for cost in (0.0, COST):
            host.mhh_set_merge_mode(1)
            host.mhh_set_label_cost(cost)
            try:
                P.run_process(sc, 2 * sc.n)
                k, labels, ms = P.run_process(sc, 2 * sc.n)
                steps, drops, members, gone = drop_log()
                j = joins()
            finally:
                host.mhh_set_merge_mode(-1)
                host.mhh_set_label_cost(0.0)
            C.CDLL(None).fflush(None)
            if k < 0:
                print(f"{n} / {k_true}  label cost {cost:g}: Process() failed", flush=True)
                continue
            q = mh.synth.agreement(sc.gt_label, labels)
            print(f"{n:6d} / {k_true:2d}  label cost {cost:4g}: clusters {k:2d}  planes recovered {q['planes_recovered']:2d}/{k_true}  ARI {q['ari']:.4f}  "
                  f"Process() {ms:8.2f} ms  joins {j}  drop steps {steps}, drops {drops} ({members} members, {gone} to the outlier label)", flush=True)
    print(flush=True)


def barrsmith():
    print("== 3. barrsmith from the raw file (load filter 2 px, point-to-line distance, DLT route, MERGE_ENERGY), compared on the rows both kept ==", flush=True)
    print("   (recorded for MERGE_ENERGY without a label cost, profiles/merge_energy_probe.txt: clusters median 8.5, planes recovered median 2, ARI median 0.826)", flush=True)
    import barrsmith_agreement as BA
    pts, ref_rows, ref_labels = BA.kept_correspondences(with_rows=True)
    for cost in (0.0, 10.0, 20.0, 40.0):
        rows_out = []
        host.mhh_set_merge_mode(1)
        host.mhh_set_label_cost(cost)
        try:
            for seed in P.SEEDS:
                rows, labels, k, _ = BA.harness_route(pts, "dlt", seed)
                steps, drops, members, gone = drop_log()
                j = joins()
                full = np.full(len(pts), -2, dtype=int)
                full[rows] = labels
                ours = full[ref_rows]
                both = ours > -2
                ari = BA.agreement(ours[both], ref_labels[both])["ari_reference_inliers"] if k > 0 else float("nan")
                planes = mh.synth.agreement(ref_labels[both], ours[both])["planes_recovered"] if k > 0 else 0
                rows_out.append((int(k), ari, int(planes), j, drops))
                print(f"label cost {cost:4g} seed {seed:5d}: {k} clusters, {planes}/5 of the reference's planes recovered, ARI on the reference's "
                      f"inliers {ari:.3f}; joins {j}, drops {drops} ({members} members, {gone} to the outlier label) in {steps} drop steps", flush=True)
        finally:
            host.mhh_set_merge_mode(-1)
            host.mhh_set_label_cost(0.0)
        C.CDLL(None).fflush(None)
        aris, ks, ps = sorted(r[1] for r in rows_out), sorted(r[0] for r in rows_out), sorted(r[2] for r in rows_out)
        print(f"   => label cost {cost:g}: clusters {[r[0] for r in rows_out]} (median {statistics.median(ks)}, min {ks[0]}, max {ks[-1]}; the reference has 5 planes), "
              f"planes recovered {[r[2] for r in rows_out]} (median {statistics.median(ps)}, min {ps[0]}, max {ps[-1]}), "
              f"ARI median {statistics.median(aris):.3f} min {aris[0]:.3f} max {aris[-1]:.3f}, joins {[r[3] for r in rows_out]}, drops {[r[4] for r in rows_out]}",
              flush=True)
    print(flush=True)


if "1" in PARTS:
    timings()
if "2" in PARTS:
    synthetic()
if "3" in PARTS:
    barrsmith()
