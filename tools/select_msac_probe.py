#!/usr/bin/env python3
"""What the greedy selection ranked by MSAC weight (mh_select_greedy_msac, csrc/select.hip) costs and buys, on one MI355X:

  select   50 000 points x 100 000 DLT hypotheses (configs[4]) in ONE process: wall time of mh_select_greedy and of
           mh_select_greedy_msac (need 20, 32 models, all points in the support set), the calls interleaved, with refitted winners
           (mh_set_tuning key 30) off and on.  Median of 20 with min and max; per round = total / rounds run (the models selected,
           plus the round that finds nobody when fewer than 32 were); and the kernel time of the scoring launches inside
           (mh_profile_get(MH_K_SCORE)) of one more call each.
  quality  Process() of the host class by the default route, F given, count against MSAC at equal seeds: the three synthetic
           scenes of profiles/sampler_probe.txt (seed 1234), the legacy_r04 generator (planes inside each other's threshold) at
           5 000 / 3 and 20 000 / 6: planes recovered, ARI, wall time of the second call and the median of five more.
  barrsmith  the raw barrsmith file through the harness route of tools/barrsmith_agreement.py (load filter 2 px, point-to-line
           distance, DLT route) over the twelve seeds of profiles/r06_barrsmith_agreement.txt, count against MSAC.

  python tools/select_msac_probe.py | grep -v '^\[Multi-H\]' > profiles/select_msac_probe.txt      (the host class logs to stdout)
Without an argument the parts run one after the other, each as a child process under a time limit of its own, the next only if
the one before ended well."""
import ctypes as C
import importlib
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIMITS = {"select": 180, "quality": 300, "barrsmith": 200}            # seconds
SEEDS12 = (1234, 7, 99, 1, 2, 3, 4, 5, 6, 8, 9, 10)


def _host():
    host = C.CDLL(os.path.join(ROOT, "multi-h_amd", "libmultih_host.so"))
    host.mhh_set_selection_score.argtypes = [C.c_int]
    host.mhh_set_selection_score.restype = None
    return host


def select():
    mh = importlib.import_module("multi-h_amd")
    n, m, thr2, need, models = 50000, 100000, 2.2 * 2.2, 20, 32
    sc = mh.synth.make_scene(n, 10, seed=1234, with_neighbours=False)
    print(f"== mh_select_greedy / mh_select_greedy_msac, {n} points x {m} DLT hypotheses, need {need}, up to {models} models (wall time) ==", flush=True)
    with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
        e.set_correspondences(sc.src, sc.dst, sc.aff)
        e.set_epipolar(sc.F, sc.e2)
        e.propose_dlt4(1234, 0, m)
        calls = (("mh_select_greedy", lambda: e.select_greedy(thr2, need, models)),
                 ("mh_select_greedy_msac", lambda: e.select_greedy_msac(thr2, need, models)))
        for refit in (0, 1):
            e.set_tuning(30, refit)
            ts, out = {name: [] for name, _ in calls}, {}
            for name, call in calls:                        # warm-up: allocations, code objects
                out[name] = call()
            for _ in range(20):
                for name, call in calls:
                    e.synchronize()
                    t0 = time.perf_counter()
                    call()
                    ts[name].append((time.perf_counter() - t0) * 1e3)
            for name, call in calls:
                t, k = ts[name], len(out[name][1])
                rounds = k + (1 if k < models else 0)
                e.profile_reset()
                e.profile_enable(True)
                call()
                e.synchronize()
                launches, ms = e.profile_get(mh.capi.K_SCORE)
                e.profile_enable(False)
                print(f"key 30 = {refit}  {name:22s}: {k} models in {rounds} rounds, median of {len(t)} calls {statistics.median(t):.3f} ms "
                      f"(min {min(t):.3f}, max {max(t):.3f}), per round {statistics.median(t) / rounds:.3f} ms; scoring launches {launches}, "
                      f"{ms:.3f} ms in all", flush=True)
            c, w = out["mh_select_greedy"], out["mh_select_greedy_msac"]
            print(f"key 30 = {refit}  by count : positions {c[1].tolist()[:10]} counts {c[2].tolist()[:10]}")
            print(f"key 30 = {refit}  by weight: positions {w[1].tolist()[:10]} counts {w[2].tolist()[:10]} weights {w[3].tolist()[:10]}", flush=True)
        e.set_tuning(30, 0)


def _process(host, sc, hyp, seed=1234):
    dp = C.POINTER(C.c_double)
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((256, 9))
    it, en, secs = C.c_int(0), C.c_double(0), C.c_double(0)
    src, dst, aff, F, e2 = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff, sc.F, sc.e2))
    t0 = time.perf_counter()
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, F.ctypes.data_as(dp),
                             e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5), 20,
                             C.c_ulonglong(seed), hyp, 32, 20, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 256, C.byref(it), C.byref(en), C.byref(secs), 0, 4)
    return k, labels, (time.perf_counter() - t0) * 1e3


def quality():
    mh = importlib.import_module("multi-h_amd")
    host = _host()
    scenes = [(50000, 10, False), (20000, 6, False), (5000, 3, False), (20000, 6, True), (5000, 3, True)]
    print("== Process(), default route, F given, seed 1234: count against MSAC selection ==", flush=True)
    for points, planes, legacy in scenes:
        sc = mh.synth.make_scene(points, planes, seed=1234, with_neighbours=False, legacy_r04=legacy)
        for score, name in ((0, "count"), (1, "msac")):
            host.mhh_set_selection_score(score)
            try:
                runs = [_process(host, sc, 2 * points) for _ in range(7)]
            finally:
                host.mhh_set_selection_score(-1)
            k, labels, _ = runs[0]
            if k < 0:
                print(f"{points:6d} / {planes:2d}{' legacy_r04' if legacy else '':11s} {name:5s}: Process() failed", flush=True)
                continue
            q = mh.synth.agreement(sc.gt_label, labels)
            ms = [r[2] for r in runs]
            print(f"{points:6d} / {planes:2d}{' legacy_r04' if legacy else '':11s} {name:5s}: clusters {k:2d}  planes recovered {q['planes_recovered']:2d}/{planes}  "
                  f"ARI {q['ari']:.4f}  second call {ms[1]:.2f} ms, median of the five after it {statistics.median(ms[2:]):.2f} ms", flush=True)


def barrsmith():
    B = importlib.import_module("barrsmith_agreement")
    host = _host()
    pts, ref_rows, ref_labels = B.kept_correspondences(with_rows=True)
    print("== raw barrsmith file, harness route (load filter 2 px, point-to-line distance, DLT route), twelve seeds ==", flush=True)
    res = {}
    for score, name in ((0, "count"), (1, "msac")):
        res[name] = []
        for seed in SEEDS12:
            host.mhh_set_selection_score(score)
            try:
                t0 = time.perf_counter()
                rows, labels, k, _ = B.harness_route(pts, "dlt", seed, 2.0, 1)
                ms = (time.perf_counter() - t0) * 1e3
            finally:
                host.mhh_set_selection_score(-1)
            full = np.full(len(pts), -2, dtype=int)
            full[rows] = labels
            ours = full[ref_rows]
            both = ours > -2
            ari = B.agreement(ours[both], ref_labels[both])["ari_reference_inliers"] if k > 0 else float("nan")
            res[name].append((k, ari))
            print(f"{name:5s} seed {seed:5d}: {k} planes, ARI on the reference's inliers {ari:.3f}, route wall time {ms:.1f} ms", flush=True)
    for name, r in res.items():
        aris = sorted(a for _, a in r)
        print(f"   => {name}: planes {[k for k, _ in r]}, median ARI {statistics.median(aris):.3f}, min {aris[0]:.3f}, max {aris[-1]:.3f}", flush=True)


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else ""
    if part in LIMITS:
        {"select": select, "quality": quality, "barrsmith": barrsmith}[part]()
    else:
        for part in LIMITS:
            r = subprocess.run(["timeout", "-k", "10", str(LIMITS[part]), sys.executable, os.path.abspath(__file__), part])
            if r.returncode != 0:
                print(f"{part}: exit status {r.returncode}; the parts after it were not run", flush=True)
                sys.exit(r.returncode)
