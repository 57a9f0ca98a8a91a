#!/usr/bin/env python3
"""What the homography refit (mh_refit_homography, csrc/refit_h.hip; MultiH::SetTailRefit) costs and buys, on one MI355X:

  call   50 000 points of one plane (25 % outliers, 0.5 px noise): wall time of one mh_refit_homography call (copy in, ONE
         launch, copies out, synchronise) for 1 and for 3 iterations, from the best-supported of 1 000 DLT hypotheses.  The
         first call of the process is left out; median of 20, in two alternating rounds of ten.  And what the refit does to
         the model: inliers at thr^2 and the RMS distance between H p and H_true p over the plane's points, before and after.
  tail   Process() on the same scene through the host class (4 000 hypotheses; one plane: the run ends in the degenerate
         tail), refit off and refit 3: wall time of the second call and the median of the five after it; labelled points and
         the same RMS.  MH_PARENT_LIBS=<dir with the parent commit's libmultih_host.so and libmultih_hip.so> adds the parent's
         library for "off", so that this build's "off" has a yardstick with the parent's own spread.

  python tools/tail_refit_probe.py | grep -v '^\[Multi-H\]' > profiles/tail_refit_probe.txt      (the host class reports its stages on stdout)
Every part is a child process under a time limit of its own (two libraries of the same name cannot share a process); the
tail parts alternate parent / off / on, twice; nothing more is started after a part that did not end well."""
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
LIMIT = 240                                        # seconds per part
N, THR = 50000, 2.2


def scene():
    mh = importlib.import_module("multi-h_amd")
    return mh, mh.synth.make_scene(N, 1, seed=1234, with_neighbours=False)


def rms_to_truth(mh, sc, H):
    g = sc.gt_label == 0
    d = mh.synth.apply_h(H, sc.src[g]) - mh.synth.apply_h(sc.H_true[0], sc.src[g])
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


def call():
    mh, sc = scene()
    thr2 = THR * THR
    print(f"== mh_refit_homography, {N} points, one plane ({int((sc.gt_label == 0).sum())} of them on it), thr {THR} px (wall time per call) ==", flush=True)
    with mh.Engine(0, 2.6, THR, 0.005, 0.5, 20) as e:
        e.set_correspondences(sc.src, sc.dst)
        e.propose_dlt4(1234, 0, 1000)
        cnt = e.score(thr2)
        H0 = e.get_model(int(np.argmax(cnt)))
        e.refit_homography(H0, thr2, 1)                     # the first call of the process: buffers, code object
        ts = {1: [], 3: []}
        for _ in range(2):
            for it in (1, 3):
                for _ in range(10):
                    t0 = time.perf_counter()
                    e.refit_homography(H0, thr2, it)
                    ts[it].append((time.perf_counter() - t0) * 1e3)
        for it in (1, 3):
            t = ts[it]
            print(f"iterations {it}: median of {len(t)} calls {statistics.median(t):.4f} ms (min {min(t):.4f}, max {max(t):.4f})", flush=True)
        for it in (0, 1, 3, 16):
            H, mask, inl, acc = e.refit_homography(H0, thr2, it)
            print(f"iterations {it:2d}: fits accepted {acc}, inliers {inl}, RMS to the true H over the plane {rms_to_truth(mh, sc, H):.4f} px", flush=True)


def tail(mode):
    """mode: off | on | parent (the library of MH_PARENT_LIBS, refit off)"""
    mh, sc = scene()
    libdir = os.environ["MH_PARENT_LIBS"] if mode == "parent" else os.path.join(ROOT, "multi-h_amd")
    host = C.CDLL(os.path.join(libdir, "libmultih_host.so"))
    dp = C.POINTER(C.c_double)
    src, dst, aff = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff))

    def run():
        labels = np.full(sc.n, -7, dtype=np.int32)
        Hout = np.zeros((8, 9))
        t0 = time.perf_counter()
        k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n,
                                 None, None, C.c_double(2.6), C.c_double(THR), C.c_double(0.005), C.c_double(0.5), 20,
                                 C.c_ulonglong(99), 4000, 8, 0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                                 Hout.ctypes.data_as(dp), 8, None, None, None, 0, 4)
        return k, (time.perf_counter() - t0) * 1e3, int((labels == 0).sum()), Hout[0].copy()

    if mode == "on":
        host.mhh_set_tail_refit(3)
    try:
        runs = [run() for _ in range(7)]
    finally:
        if mode == "on":
            host.mhh_set_tail_refit(-1)
    ms = [r[1] for r in runs]
    if runs[0][0] != 1:
        sys.exit(f"tail {mode}: Process() returned {runs[0][0]} clusters, not the degenerate tail's one")
    print(f"tail refit {mode:6s}: label-0 points {runs[0][2]}, RMS to the true H {rms_to_truth(mh, sc, runs[0][3]):.4f} px, first call {ms[0]:.2f} ms, "
          f"second call {ms[1]:.2f} ms, median of the five after it {statistics.median(ms[2:]):.2f} ms (min {min(ms[2:]):.2f}, max {max(ms[2:]):.2f})",
          flush=True)


if __name__ == "__main__":
    part = sys.argv[1:] if len(sys.argv) > 1 else []
    if part == ["call"]:
        call()
    elif len(part) == 2 and part[0] == "tail":
        tail(part[1])
    else:
        modes = (["parent"] if os.environ.get("MH_PARENT_LIBS") else []) + ["off", "on"]
        for i, p in enumerate([["call"]] + [["tail", m] for m in modes] * 2):
            if i == 1:
                print(f"\n== Process() ending in the degenerate tail: {N} points, one plane, 4 000 hypotheses (wall time of the whole call) ==")
            sys.stdout.flush()
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + p, timeout=LIMIT)
            if r.returncode != 0:
                sys.exit(f"tail_refit_probe: part {' '.join(p)} ended with status {r.returncode}; nothing more is started")
