#!/usr/bin/env python3
"""The N-point DLT re-estimator and the route without epipolar geometry on the GPU.

  1. mh_reestimate's kernel time under "haf", "3pt" and "dlt" at 50 000 points x 11 labels and 20 000 points x 540 labels, by the
     engine's per-kernel events (mh_profile_*), the median of REPS runs (default 21).  No affinities and no F are set for "dlt".
  2. The three-motion scene of the tests (tests/reestimate_dlt_numpy.py::three_motions: three independently moving planes) at
     1 200 and 20 000 points through mhh_run_process: planes recovered, ARI and the wall time of Process() (median of RUNS,
     default 5) by the epipolar-free route and by the default route, whose one estimated F is wrong by construction on this
     scene: whatever it returns is recorded as it comes.

Prints plain text (the host class logs its own "[Multi-H]" and "Iteration" lines to stdout beside it);
profiles/epipolar_free_probe.txt holds these lines from one MI355X, the kernel's resource line and the flagship benchmark's
this / parent / this record of the same sessions."""
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
mh = importlib.import_module("multi-h_amd")
import reestimate_dlt_numpy as D                                      # noqa: E402

REPS = int(os.environ.get("REPS", 21))
RUNS = int(os.environ.get("RUNS", 5))
K_REESTIMATE = 5


def reestimate_us(n, nh, estimator):
    sc = mh.synth.make_scene(n, 10, seed=1234, with_neighbours=False)
    rng = np.random.default_rng(7)
    lab = np.where(sc.gt_label >= 0, sc.gt_label, rng.integers(-1, nh, size=n)).astype(np.int32)
    H0 = np.tile(sc.H_true, ((nh + 9) // 10, 1))[:nh]
    with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
        if estimator == "dlt":
            e.set_correspondences(sc.src, sc.dst)
        else:
            e.set_correspondences(sc.src, sc.dst, sc.aff)
            e.set_epipolar(sc.F, sc.e2)
        e.set_estimator(estimator)
        e.profile_enable(True)
        out = []
        for r in range(REPS + 2):
            e.set_models(H0)
            e.profile_reset()
            e.reestimate(lab)
            e.synchronize()
            k, ms = e.profile_get(K_REESTIMATE)
            if r >= 2:
                out.append(ms / max(k, 1))
    return 1e3 * float(np.median(out))


def run_process(host, sc):
    dp = C.POINTER(C.c_double)
    labels = np.full(sc.n, -1, dtype=np.int32)
    Hout = np.zeros((64, 9))
    src, dst, aff = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff))
    t0 = time.perf_counter()
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, None, None,
                             C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(5), 4000, 16,
                             0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)), Hout.ctypes.data_as(dp), 64, None, None, None,
                             0, 4)
    return k, labels, 1e3 * (time.perf_counter() - t0)


def main():
    print(f"reestimate kernel time, median of {REPS} (us)")
    for n, nh in ((50000, 11), (20000, 540)):
        row = "  ".join(f"{est} {reestimate_us(n, nh, est):8.1f}" for est in ("haf", "3pt", "dlt"))
        print(f"  {n:6d} points x {nh:3d} labels:  {row}", flush=True)
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_epipolar_free.argtypes, host.mhh_set_epipolar_free.restype = [C.c_int], None
    print(f"three-motion scene through Process(), wall time the median of {RUNS} runs after one warm-up")
    for n in (1200, 20000):
        sc = D.three_motions(n)
        for route, flag in (("epipolar-free", 1), ("default", 0)):
            try:
                host.mhh_set_epipolar_free(flag)
                times, last = [], None
                for r in range(RUNS + 1):
                    last = run_process(host, sc)
                    if r >= 1:
                        times.append(last[2])
            finally:
                host.mhh_set_epipolar_free(0)
            C.CDLL(None).fflush(None)
            k, labels, _ = last
            if k < 0:
                print(f"  {n:6d} points, {route:13s}: Process() failed", flush=True)
                continue
            got = mh.synth.agreement(sc.gt_label, labels)
            print(f"  {n:6d} points, {route:13s}: {k} models, planes {got['planes_recovered']} of {got['planes']}, "
                  f"ARI {got['ari']:.4f}, Process() {np.median(times):.1f} ms", flush=True)


if __name__ == "__main__":
    main()
