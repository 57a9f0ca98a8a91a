#!/usr/bin/env python3
"""What the distance-weighted smoothness (mh_set_smoothness_weights(MH_SMOOTH_CAUCHY), MultiH::SetSmoothnessWeights,
multih_harness --smoothness cauchy:RHO[:QMAX]) costs and does, next to the uniform weights, on one MI355X:

  1. the weight pass on a resident graph (16 nearest hits within 200 px) at 50 000 and 20 000 points: host time of one
     mh_set_smoothness_weights call, median of REPEAT — under CAUCHY a 4-byte clear, k_arc_weights, a 4-byte read-back and the
     wait for it; under UNIFORM k_row_wsum and the wait.  The difference of the two is what the rule adds to a build.
  2. the neighbourhood build (mh_build_neighbors_knn_radius, 16 hits within 200 px, 50 000 points) with the rule UNIFORM, by this
     library and by another build of the ABI named in PARENT_LIB (the parent commit's), each in a process of its own, twice in
     alternation: median of REPEAT builds.
  3. one cold mh_labeling_step on the three labeling scenes of the bench line (50 000 x 11 labels) and Process() on the synthetic
     scenes of tools/data_term_probe.py, under UNIFORM and under CAUCHY with rho in {20, 50, 100}, q_max in {8, 16}, at lambda 0.5
     and at lambda / sqrt(q_max): planes recovered, ARI.
  4. barrsmith (tests/golden/barrsmith.npz) over the twelve seeds of profiles/r06_barrsmith_agreement.txt, on the reference's rows
     and from the raw file (DLT route): planes, ARI on the reference's inliers against the reference's labels.

  python tools/smooth_weights_probe.py > profiles/smooth_weights_probe.txt
Env: REPEAT (20), PARTS ("1234"), PARENT_LIB (part 2; without it only this library is timed)."""
import ctypes as C
import importlib
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
mh = importlib.import_module("multi-h_amd")

REPEAT = int(os.environ.get("REPEAT", 20))
PARTS = os.environ.get("PARTS", "1234")
SEEDS = (1234, 7, 99, 1, 2, 3, 4, 5, 6, 8, 9, 10)
LAM = 0.5
dp = C.POINTER(C.c_double)


def configs():
    """(name, (rule, rho, q_max) or None, lambda): UNIFORM, then the sweep at lambda and at lambda / sqrt(q_max)."""
    out = [("uniform", None, LAM)]
    for q in (8, 16):
        for rho in (20.0, 50.0, 100.0):
            out.append((f"cauchy rho {rho:5.1f} q_max {q:2d} lambda {LAM:.4f}", (1, rho, q), LAM))
            out.append((f"cauchy rho {rho:5.1f} q_max {q:2d} lambda {LAM / math.sqrt(q):.4f}", (1, rho, q), LAM / math.sqrt(q)))
    return out


def build_time_child():
    """(part 2, in a process of its own: MH_LIB names the library) median ms of REPEAT neighbourhood builds."""
    sc = mh.synth.make_scene(50000, 10, seed=1234, with_neighbours=False)
    with mh.Engine(0, 2.6, 2.2, 0.005, LAM, 20) as e:
        e.set_correspondences(sc.src, sc.dst, sc.aff)
        for _ in range(3):
            e.build_neighbors_knn(16, radius=200.0)
        ts = []
        for _ in range(REPEAT):
            t0 = time.perf_counter()
            e.build_neighbors_knn(16, radius=200.0)
            ts.append((time.perf_counter() - t0) * 1e3)
        nnz = len(e.get_sym_graph()[1])
    print(f"{statistics.median(ts):.4f} {min(ts):.4f} {max(ts):.4f} {nnz}")


def weight_pass():
    print(f"== 1. mh_set_smoothness_weights on a resident graph (16 hits within 200 px), host time of the call, median of {REPEAT} ==", flush=True)
    for n in (50000, 20000):
        sc = mh.synth.make_scene(n, 10, seed=1234, with_neighbours=False)
        with mh.Engine(0, 2.6, 2.2, 0.005, LAM, 20) as e:
            e.set_correspondences(sc.src, sc.dst, sc.aff)
            e.build_neighbors_knn(16, radius=200.0)
            nnz = len(e.get_sym_graph()[1])
            t = {"cauchy": [], "uniform": []}
            for k in range(REPEAT + 3):
                for rule in ("cauchy", "uniform"):
                    t0 = time.perf_counter()
                    e.set_smoothness_weights(rule, 50.0, 16)
                    if k >= 3:
                        t[rule].append((time.perf_counter() - t0) * 1e3)
            c, u = statistics.median(t["cauchy"]), statistics.median(t["uniform"])
            print(f"{n:6d} points, {nnz} arcs: CAUCHY {c:.4f} ms (min {min(t['cauchy']):.4f}, max {max(t['cauchy']):.4f}), "
                  f"UNIFORM {u:.4f} ms (min {min(t['uniform']):.4f}, max {max(t['uniform']):.4f}), difference {c - u:+.4f} ms", flush=True)
    print(flush=True)


def build_times():
    print(f"== 2. neighbourhood build, 50 000 points, 16 hits within 200 px, rule UNIFORM, median of {REPEAT} builds per process ==", flush=True)
    libs = [("this library", mh.LIB_PATH)]
    if os.environ.get("PARENT_LIB"):
        libs.append(("parent commit", os.path.abspath(os.environ["PARENT_LIB"])))
    for rnd in range(2):
        for name, path in libs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--build-time-child"], env={**os.environ, "MH_LIB": path},
                                 capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                print(f"{name}: failed: {out.stderr[-300:]}", flush=True)
                continue
            med, lo, hi, nnz = out.stdout.split()
            print(f"round {rnd}, {name:13s}: median {med} ms (min {lo}, max {hi}), {nnz} arcs", flush=True)
    print(flush=True)


def _host():
    host = C.CDLL(os.path.join(ROOT, "multi-h_amd", "libmultih_host.so"))
    host.mhh_set_smoothness_weights.argtypes = [C.c_int, C.c_double, C.c_int]
    host.mhh_set_smoothness_weights.restype = None
    return host


def process(host, sc, H0, hyp, lam, seed=1234):
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((256, 9))
    it, en, secs = C.c_int(0), C.c_double(0), C.c_double(0)
    src, dst, aff, F, e2 = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff, sc.F, sc.e2))
    H0c = None if H0 is None else np.ascontiguousarray(H0)
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, F.ctypes.data_as(dp),
                             e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(lam), 20,
                             C.c_ulonglong(seed), hyp, 32, 20, None if H0c is None else H0c.ctypes.data_as(dp),
                             0 if H0c is None else H0c.shape[0], labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 256, C.byref(it), C.byref(en), C.byref(secs), 0, 4)
    return k, labels, it.value, en.value


def synthetic():
    print("== 3a. one cold mh_labeling_step, 50 000 sites x 11 labels, the three labeling scenes of the bench line ==", flush=True)
    for legacy, sep, what in ((False, None, "planes 13 px apart"), (False, 2.0, "planes 2 px apart"), (True, None, "r04 generator")):
        kw = {} if sep is None else {"plane_separation": sep}
        sc = mh.synth.make_scene(50000, 10, seed=1234, legacy_r04=legacy, **kw)
        H = sc.H_true * (1.0 + np.random.default_rng(0).normal(0, 1e-4, size=sc.H_true.shape))
        for name, rule, lam in configs():
            with mh.Engine(0, 2.6, 2.2, 0.005, lam, 20) as e:
                e.set_correspondences(sc.src, sc.dst, sc.aff)
                e.set_epipolar(sc.F, sc.e2)
                if rule:
                    e.set_smoothness_weights(*rule)
                e.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
                ts = []
                for _ in range(4):
                    e.set_models(H)
                    t0 = time.perf_counter()
                    lab, energy, cycles = e.labeling_step(False, np.full(sc.n, -1, np.int32))
                    ts.append((time.perf_counter() - t0) * 1e3)
                q = mh.synth.agreement(sc.gt_label, lab)
                print(f"{what:20s} {name:44s}: energy {int(energy):10d}  cycles {cycles}  planes recovered {q['planes_recovered']:2d}/10  "
                      f"ARI {q['ari']:.4f}  {statistics.median(ts[1:]):7.3f} ms", flush=True)
    print(flush=True)
    print("== 3b. Process() on synthetic scenes with ground truth (seed 1234, 10 planes, post-filter on, at most 20 iterations) ==", flush=True)
    host = _host()
    for points, legacy, what in ((10000, True, "r04 generator"), (50000, True, "r04 generator"), (50000, False, "separated (configs[4])")):
        sc = mh.synth.make_scene(points, 10, seed=1234, with_neighbours=False, legacy_r04=legacy)
        rng = np.random.default_rng(1234)
        H0 = [sc.H_true * (1.0 + rng.normal(0, 1e-4, size=sc.H_true.shape))]
        for _ in range(5):
            k = rng.integers(0, 10)
            H0.append(sc.H_true[k:k + 1] * (1.0 + rng.normal(0, 2e-4, size=(1, 9))))
        for _ in range(2):
            H0.append((np.eye(3) + rng.normal(0, 0.05, size=(3, 3))).reshape(1, 9))
        H0 = np.ascontiguousarray(np.concatenate(H0))
        for init, h0, hyp in (("initial models of plane_trace", H0, 0), ("DLT proposals", None, 2 * points)):
            for name, rule, lam in configs():
                host.mhh_set_smoothness_weights(*(rule or (-1, 0.0, 16)))
                try:
                    k, labels, it, en = process(host, sc, h0, hyp, lam)
                finally:
                    host.mhh_set_smoothness_weights(-1, 0.0, 16)
                if k < 0:
                    print(f"{points:6d} {what:24s} {init:30s} {name:44s}: Process() failed", flush=True)
                    continue
                q = mh.synth.agreement(sc.gt_label, labels)
                print(f"{points:6d} {what:24s} {init:30s} {name:44s}: clusters {k:2d}  planes recovered {q['planes_recovered']:2d}/10  "
                      f"ARI {q['ari']:.4f}  iterations {it:2d}  LabelingSteps {host.mhh_get_labeling_steps():2d}  energy {en:.0f}", flush=True)
    print(flush=True)


def barrsmith():
    import barrsmith_agreement as BA
    print("== 4. barrsmith: agreement with the reference's labels (ARI on the reference's inliers), DLT route, twelve seeds ==", flush=True)
    host = _host()
    corr, ref, matched, total = BA.kept_correspondences()
    e = mh.Engine(0, 2.6, 2.2, 0.005, LAM, 20)
    e.set_correspondences(corr[:, 0:2], corr[:, 2:4], corr[:, 4:8])
    F, e2, mask, inl = e.estimate_fundamental(1234 ^ 0xf00d, 4000, 2.6)
    e.close()
    pts, ref_rows, ref_labels = BA.kept_correspondences(with_rows=True)
    nan = {"ari_reference_inliers": float("nan")}
    for name, rule, lam in configs():
        rows_ref, rows_raw = [], []
        host.mhh_set_smoothness_weights(*(rule or (-1, 0.0, 16)))
        try:
            for seed in SEEDS:
                k, labels, it, en = BA.run("dlt", corr, F, e2, seed=seed, lam=lam)
                rows_ref.append((int(k), (BA.agreement(labels, ref) if k > 0 else nan)["ari_reference_inliers"]))
                kept, labels, k, stages = BA.harness_route(pts, "dlt", seed, 2.0, 1, lam=lam)
                full = np.full(len(pts), -2, dtype=int)
                full[kept] = labels
                ours = full[ref_rows]
                both = ours > -2
                rows_raw.append((int(k), (BA.agreement(ours[both], ref_labels[both]) if k > 0 else nan)["ari_reference_inliers"]))
        finally:
            host.mhh_set_smoothness_weights(-1, 0.0, 16)
        for tag, rows in (("reference's rows", rows_ref), ("raw file", rows_raw)):
            aris = sorted(r[1] for r in rows)
            print(f"{name:44s} {tag:16s}: planes {[r[0] for r in rows]}, ARI median {statistics.median(aris):.3f} min {aris[0]:.3f} "
                  f"max {aris[-1]:.3f}", flush=True)
    print(flush=True)


if "--build-time-child" in sys.argv:
    build_time_child()
    sys.exit(0)
if "1" in PARTS:
    weight_pass()
if "2" in PARTS:
    build_times()
if "3" in PARTS:
    synthetic()
if "4" in PARTS:
    barrsmith()
