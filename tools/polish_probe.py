#!/usr/bin/env python3
"""What the Levenberg-Marquardt polish (mh_polish_homographies, csrc/polish_h.hip; MultiH::SetTailPolish / SetModelPolish)
costs and buys, on one MI355X:

  call     wall time of one mh_polish_homographies call (labels and models in, ONE launch, copies out, synchronise) with
           max_iterations = 10; the first call of the process is left out; median of 20.  Three shapes:
             50 000 points / one plane, m = 1   the plane's points labelled 0, from the best-supported of 1 000 DLT hypotheses
                                                and from its one-round refit (mh_refit_homography);
             50 000 points / 10 labels          ten planes, the ground-truth labels, every model a pixel off its plane;
             20 000 points / 540 labels         one plane, label = index mod 540 (37 members each), every model a pixel off.
           And what the polish does to the models: iterations run, steps accepted, S before and after, and the RMS distance
           between H p and H_true p over the label's points before and after (the mean over the labels).
  process  Process() through the host class, wall time of the second call and the median of the five after it:
             tail    50 000 points, one plane, 4 000 hypotheses (the run ends in the degenerate tail): off, and
                     SetTailRefit(1) + SetTailPolish(10), OpenCV's sequence;
             final   20 000 points, 6 planes, 4 000 hypotheses: off and SetModelPolish(10).
           MH_PARENT_LIBS=<dir with the parent commit's libmultih_host.so and libmultih_hip.so> adds the parent's library for
           "off", so that this build's "off" has a yardstick with the parent's own spread.

  python tools/polish_probe.py | grep -v '^\\[Multi-H\\]' > profiles/polish_probe.txt      (the host class reports its stages on stdout)
Every part is a child process under a time limit of its own (two libraries of the same name cannot share a process); the
process parts alternate parent / off / on, twice; nothing more is started after a part that did not end well."""
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
THR = 2.2
SCENES = {"tail": (50000, 1, 8), "final": (20000, 6, 32)}          # points, planes, max models


def rms_to_truth(mh, sc, H, plane, sel=None):
    g = (sc.gt_label == plane) if sel is None else sel
    d = mh.synth.apply_h(H, sc.src[g]) - mh.synth.apply_h(sc.H_true[plane], sc.src[g])
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


def off_by_a_pixel(H, rng):
    H = np.array(H, dtype=np.float64).reshape(9) / H.reshape(9)[8]
    H[2] += rng.normal(0, 1.0)
    H[5] += rng.normal(0, 1.0)
    return H


def timed(e, labels, H, it=10):
    e.polish_homographies(labels, H, it)                   # the first call of the process: buffers, code object
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        out = e.polish_homographies(labels, H, it)
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def report(name, mh, sc, labels, planes_of, H_in, out, ts):
    H, cost, info = out
    m = H_in.shape[0]
    before = np.mean([rms_to_truth(mh, sc, H_in[k], planes_of[k], labels == k) for k in range(m)])
    after = np.mean([rms_to_truth(mh, sc, H[k], planes_of[k], labels == k) for k in range(m)])
    print(f"{name}: median of {len(ts)} calls {statistics.median(ts):.4f} ms (min {min(ts):.4f}, max {max(ts):.4f}); iterations "
          f"{info[:, 1].min()}..{info[:, 1].max()}, steps accepted {info[:, 2].min()}..{info[:, 2].max()}, sum of S {cost[:, 0].sum():.6g} -> "
          f"{cost[:, 1].sum():.6g}, mean RMS to the true H over the members {before:.4f} -> {after:.4f} px", flush=True)


def call():
    mh = importlib.import_module("multi-h_amd")
    rng = np.random.default_rng(7)
    thr2 = THR * THR
    print("== mh_polish_homographies, max_iterations 10 (wall time per call) ==", flush=True)
    sc = mh.synth.make_scene(50000, 1, seed=1234, with_neighbours=False)
    labels = np.where(sc.gt_label == 0, 0, -1).astype(np.int32)
    with mh.Engine(0, 2.6, THR, 0.005, 0.5, 20) as e:
        e.set_correspondences(sc.src, sc.dst)
        e.propose_dlt4(1234, 0, 1000)
        H0 = e.get_model(int(np.argmax(e.score(thr2)))).reshape(1, 9)
        H1 = e.refit_homography(H0, thr2, 1)[0].reshape(1, 9)
        for name, H in (("50 000 / one plane, m = 1, from the DLT winner  ", H0), ("50 000 / one plane, m = 1, from its 1-round refit", H1)):
            out, ts = timed(e, labels, H)
            report(name, mh, sc, labels, [0], H, out, ts)
        # 20 000 / 540 labels on the first 20 000 points of the same plane
        sub = np.flatnonzero(sc.gt_label == 0)[:20000]
        e.set_correspondences(sc.src[sub], sc.dst[sub])
        lab540 = (np.arange(20000) % 540).astype(np.int32)
        H540 = np.stack([off_by_a_pixel(sc.H_true[0], rng) for _ in range(540)])

        class Sub:
            src, dst, H_true, gt_label = sc.src[sub], sc.dst[sub], sc.H_true, np.zeros(20000, np.int64)
        out, ts = timed(e, lab540, H540)
        report("20 000 / 540 labels (37 members each)            ", mh, Sub, lab540, [0] * 540, H540, out, ts)
        sc10 = mh.synth.make_scene(50000, 10, seed=1234, with_neighbours=False)
        e.set_correspondences(sc10.src, sc10.dst)
        lab10 = sc10.gt_label.astype(np.int32)
        H10 = np.stack([off_by_a_pixel(sc10.H_true[k], rng) for k in range(10)])
        out, ts = timed(e, lab10, H10)
        report("50 000 / 10 labels (the ground truth's)           ", mh, sc10, lab10, list(range(10)), H10, out, ts)


def process(which, mode):
    """which: tail | final; mode: off | on | parent (the library of MH_PARENT_LIBS, everything off)"""
    mh = importlib.import_module("multi-h_amd")
    n, planes, max_models = SCENES[which]
    sc = mh.synth.make_scene(n, planes, seed=1234, with_neighbours=False)
    libdir = os.environ["MH_PARENT_LIBS"] if mode == "parent" else os.path.join(ROOT, "multi-h_amd")
    host = C.CDLL(os.path.join(libdir, "libmultih_host.so"))
    dp = C.POINTER(C.c_double)
    src, dst, aff = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff))

    def run():
        labels = np.full(sc.n, -7, dtype=np.int32)
        Hout = np.zeros((max_models, 9))
        t0 = time.perf_counter()
        k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n,
                                 None, None, C.c_double(2.6), C.c_double(THR), C.c_double(0.005), C.c_double(0.5), 20,
                                 C.c_ulonglong(99), 4000, max_models, 0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                                 Hout.ctypes.data_as(dp), max_models, None, None, None, 0, 4)
        return k, (time.perf_counter() - t0) * 1e3, labels, Hout[:max(k, 0)].copy()

    if mode == "on":
        if which == "tail":
            host.mhh_set_tail_refit(1)
            host.mhh_set_tail_polish(10)
        else:
            host.mhh_set_model_polish(10)
    try:
        runs = [run() for _ in range(7)]
    finally:
        if mode == "on":
            host.mhh_set_tail_refit(-1)
            host.mhh_set_tail_polish(-1)
            host.mhh_set_model_polish(-1)
    ms = [r[1] for r in runs]
    k, _, labels, H = runs[0]
    if (which == "tail") != (k == 1) or k < 1:
        sys.exit(f"{which} {mode}: Process() returned {k} clusters")
    # a cluster's plane: the ground-truth label most of its points carry (the labels may index refined, filtered points: then
    # the clusters are compared by their models alone, over the whole of the nearest plane)
    rms = []
    for c in range(k):
        rms.append(min(rms_to_truth(mh, sc, H[c], p) for p in range(planes)))
    print(f"{which:5s} {mode:6s}: {k} clusters, mean RMS of a model to the nearest true H {np.mean(rms):.4f} px, first call {ms[0]:.2f} ms, "
          f"second call {ms[1]:.2f} ms, median of the five after it {statistics.median(ms[2:]):.2f} ms (min {min(ms[2:]):.2f}, max {max(ms[2:]):.2f})",
          flush=True)


if __name__ == "__main__":
    part = sys.argv[1:] if len(sys.argv) > 1 else []
    if part == ["call"]:
        call()
    elif len(part) == 3 and part[0] == "process":
        process(part[1], part[2])
    else:
        modes = (["parent"] if os.environ.get("MH_PARENT_LIBS") else []) + ["off", "on"]
        parts = [["call"]] + [["process", w, m] for w in ("tail", "final") for m in modes] * 2
        for i, p in enumerate(parts):
            if i == 1:
                print("\n== Process(): tail = 50 000 points, one plane (refit 1 + polish 10 when on); final = 20 000 points, 6 planes "
                      "(model polish 10 when on); 4 000 hypotheses (wall time of the whole call) ==")
            sys.stdout.flush()
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + p, timeout=LIMIT)
            if r.returncode != 0:
                sys.exit(f"polish_probe: part {' '.join(p)} ended with status {r.returncode}; nothing more is started")
