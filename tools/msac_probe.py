#!/usr/bin/env python3
"""What the MSAC-weighted score (mh_score_msac, csrc/msac32.hip) costs, on one MI355X:

  kernels  50 000 points x 100 000 DLT hypotheses in ONE process: kernel time (mh_profile_get) of mh_score — the yardstick: the
           same pre-test, nothing summed; by its default resident grid and by hardware dispatch (key 24 = 0), which is how
           k_msac32 is launched —, of mh_score_msac in its pre-test form, and of mh_cost_matrix — the upper reference: every
           near pair through the FP64 formula plus a 20 GB store stream.  Median of 20 launches each, interleaved in two rounds
           of ten; and the MSAC call's pairs_fp64 / pairs (mh_get_score_stats).
  tail     Process() on the single-plane scene of tests/test_gpu_msac.py (3 000 points, 35 % outliers, 4 000 hypotheses), which
           ends in the degenerate tail, under TAIL_SCORE_COUNT and TAIL_SCORE_MSAC: wall time of the second call and of five more.

  python tools/msac_probe.py > profiles/msac_probe.txt
Without an argument both parts run, each as a child process under a time limit of its own, the second only if the first ended
well."""
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
LIMITS = {"kernels": 240, "tail": 180}            # seconds


def kernels():
    mh = importlib.import_module("multi-h_amd")
    K = mh.capi
    n, m, thr2 = 50000, 100000, 2.2 * 2.2
    sc = mh.synth.make_scene(n, 10, seed=1234, with_neighbours=False)
    print(f"== mh_score / mh_score_msac / mh_cost_matrix, {n} points x {m} DLT hypotheses (kernel time, mh_profile_get) ==", flush=True)
    with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
        e.set_correspondences(sc.src, sc.dst, sc.aff)
        e.propose_dlt4(1234, 0, m)

        def timed(call, kernel):
            e.profile_reset()
            e.profile_enable(True)
            call()
            e.synchronize()
            launches, ms = e.profile_get(kernel)
            e.profile_enable(False)
            return ms / max(launches, 1)

        def score_hw():
            e.set_tuning(24, 0)
            e.score(thr2, fetch=False)
            e.set_tuning(24, 12)

        steps = (("mh_score (resident grid, default)", lambda: e.score(thr2, fetch=False), K.K_SCORE),
                 ("mh_score (hardware dispatch)", score_hw, K.K_SCORE),
                 ("mh_score_msac (pre-test form)", lambda: e.score_msac(thr2, fetch=False), K.K_SCORE),
                 ("mh_cost_matrix", lambda: e.cost_matrix(fetch_C=False, fetch_counts=False), K.K_COSTMATRIX))
        ts = {name: [] for name, _, _ in steps}
        for name, call, _ in steps:                      # warm-up: allocations, code objects
            call()
        e.synchronize()
        for _ in range(2):
            for name, call, kernel in steps:
                for _ in range(10):
                    ts[name].append(timed(call, kernel))
        for name, _, _ in steps:
            t = ts[name]
            print(f"{name:36s}: median of {len(t)} launches {statistics.median(t):.4f} ms (min {min(t):.4f}, max {max(t):.4f})", flush=True)
        cnt = e.score(thr2)
        e.score_stats(reset=True)
        cnt_m, wgt = e.score_msac(thr2)
        pairs, fp64 = e.score_stats(reset=True)
        assert np.array_equal(cnt, cnt_m)
        print(f"mh_score_msac: pairs {pairs}, pairs_fp64 {fp64} ({100.0 * fp64 / pairs:.3f} %), inlier pairs {int(cnt.sum())} "
              f"({100.0 * int(cnt.sum()) / pairs:.3f} %)", flush=True)
        e.score(thr2, fetch=False)
        pairs, fp64 = e.score_stats(reset=True)
        print(f"mh_score:      pairs {pairs}, pairs_fp64 {fp64} ({100.0 * fp64 / pairs:.3f} %)", flush=True)
        print(f"best by count: model {int(np.argmax(cnt))} (count {int(cnt.max())}, weight {int(wgt[np.argmax(cnt)])}); "
              f"best by weight: model {int(np.argmax(wgt))} (count {int(cnt[np.argmax(wgt)])}, weight {int(wgt.max())})", flush=True)


def tail():
    mh = importlib.import_module("multi-h_amd")
    host = C.CDLL(os.path.join(ROOT, "multi-h_amd", "libmultih_host.so"))
    host.mhh_set_tail_score.argtypes = [C.c_int]
    host.mhh_set_tail_score.restype = None
    dp = C.POINTER(C.c_double)
    sc = mh.synth.make_scene(3000, 1, seed=5, outlier_frac=0.35, legacy_r04=True)
    src, dst, aff = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff))
    print("== Process() ending in the degenerate tail: 3 000 points, one plane, 35 % outliers, 4 000 hypotheses (wall time) ==", flush=True)

    def run():
        labels = np.full(sc.n, -7, dtype=np.int32)
        Hout = np.zeros((8, 9))
        t0 = time.perf_counter()
        k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n,
                                 None, None, C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5), 20,
                                 C.c_ulonglong(99), 4000, 8, 0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                                 Hout.ctypes.data_as(dp), 8, None, None, None, 0, 4)
        return k, (time.perf_counter() - t0) * 1e3, int((labels == 0).sum())

    for _ in range(2):
        for score, name in ((0, "count"), (1, "msac")):
            host.mhh_set_tail_score(score)
            try:
                runs = [run() for _ in range(7)]
            finally:
                host.mhh_set_tail_score(-1)
            ms = [r[1] for r in runs]
            print(f"tail score {name:5s}: clusters {runs[0][0]}, label-0 points {runs[0][2]}, first call {ms[0]:.2f} ms, second call {ms[1]:.2f} ms, "
                  f"median of the five after it {statistics.median(ms[2:]):.2f} ms", flush=True)


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else ""
    if part == "kernels":
        kernels()
    elif part == "tail":
        tail()
    else:
        for p in ("kernels", "tail"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), p], timeout=LIMITS[p])
            if r.returncode != 0:
                sys.exit(f"msac_probe: part {p} ended with status {r.returncode}; nothing more is started")
            print(flush=True)
