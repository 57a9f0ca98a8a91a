#!/usr/bin/env python3
"""What the rising data term (mh_set_data_term(MH_DATA_TERM_RISING), MultiH::SetDataTerm, multih_harness --data-term rising)
does to the results, next to the reference's term, on one MI355X, both terms in the same process:

  1. barrsmith (tests/golden/barrsmith.npz): Process() on the reference's own 1 094 kept rows (F by the engine's 8-point
     RANSAC on them) and from the raw 2 903-row file as the harness runs it (load filter 2 px, point-to-line distance), by
     both initialisation routes, over the twelve seeds of profiles/r06_barrsmith_agreement.txt: planes, ARI on the
     reference's inliers against the reference's labels, LabelingSteps.
  2. synthetic scenes with ground truth, seed 1234, 10 planes: the r04 generator (legacy_r04=True: the scene of
     tools/plane_trace.py, planes inside each other's truncation threshold) at 10 000 and 50 000 points, and the separated
     configs[4] scene (50 000): Process() from plane_trace's initial models (perturbed truth, five near-copies, two strays)
     and by the default route (2 hypotheses per point), 20 iterations at most: clusters, planes recovered, ARI, iterations,
     LabelingSteps, Process() ms (median of REPEAT further calls).
  3. one mh_labeling_step on the three labeling scenes of the bench line (13 px, 2 px, the r04 generator; 50 000 x 11
     labels): energy, cycles, moves_solved, core_max, ms.
  4. mh_cost_matrix at 50 000 x 100 000 DLT hypotheses under either term: kernel ms (mh_profile_get), REPEAT launches.

  python tools/data_term_probe.py > profiles/data_term_probe.txt
Env: REPEAT (10), PARTS ("1234")."""
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
mh = importlib.import_module("multi-h_amd")
import barrsmith_agreement as BA  # noqa: E402

REPEAT = int(os.environ.get("REPEAT", 10))
PARTS = os.environ.get("PARTS", "1234")
SEEDS = (1234, 7, 99, 1, 2, 3, 4, 5, 6, 8, 9, 10)
TERMS = ((0, "reference"), (1, "rising"))
host = C.CDLL(os.path.join(ROOT, "multi-h_amd", "libmultih_host.so"))
host.mhh_set_data_term.argtypes = [C.c_int]
host.mhh_set_data_term.restype = None
dp = C.POINTER(C.c_double)


def summary(tag, rows):
    """rows: (planes, ari, steps) per seed."""
    aris = sorted(r[1] for r in rows)
    print(f"   => {tag}: planes {[r[0] for r in rows]}, ARI median {statistics.median(aris):.3f} min {aris[0]:.3f} max {aris[-1]:.3f} "
          f"spread {aris[-1] - aris[0]:.3f}, LabelingSteps {[r[2] for r in rows]}", flush=True)


def barrsmith():
    print("== 1. barrsmith: agreement with the reference's labels (ARI on the reference's inliers) ==", flush=True)
    corr, ref, matched, total = BA.kept_correspondences()
    e = mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20)
    e.set_correspondences(corr[:, 0:2], corr[:, 2:4], corr[:, 4:8])
    F, e2, mask, inl = e.estimate_fundamental(1234 ^ 0xf00d, 4000, 2.6)
    e.close()
    print(f"the reference's rows: {matched} of {total} matched to the input, F from them (seed 1234): {int(inl)} inliers at 2.6 px")
    for route in ("dlt", "stable_sets"):
        for term, name in TERMS:
            rows = []
            host.mhh_set_data_term(term)
            try:
                for seed in SEEDS:
                    k, labels, it, en = BA.run(route, corr, F, e2, seed=seed)
                    a = BA.agreement(labels, ref) if k > 0 else {"ari_reference_inliers": float("nan"), "ari_all": float("nan")}
                    steps = host.mhh_get_labeling_steps()
                    rows.append((int(k), a["ari_reference_inliers"], steps))
                    print(f"reference's rows, {route:12s} {name:9s} seed {seed:5d}: {k} planes, ARI on the reference's inliers {a['ari_reference_inliers']:.3f}, "
                          f"all {a['ari_all']:.3f}, LabelingSteps {steps}, energy {en:.0f}", flush=True)
            finally:
                host.mhh_set_data_term(-1)
            summary(f"reference's rows, {route}, {name}", rows)
    pts, ref_rows, ref_labels = BA.kept_correspondences(with_rows=True)
    for route in ("dlt", "stable_sets"):
        for term, name in TERMS:
            rows = []
            host.mhh_set_data_term(term)
            try:
                for seed in SEEDS:
                    kept, labels, k, stages = BA.harness_route(pts, route, seed, 2.0, 1)
                    steps = host.mhh_get_labeling_steps()
                    full = np.full(len(pts), -2, dtype=int)
                    full[kept] = labels
                    ours = full[ref_rows]
                    both = ours > -2
                    a = BA.agreement(ours[both], ref_labels[both]) if k > 0 else {"ari_reference_inliers": float("nan"), "ari_all": float("nan")}
                    rows.append((int(k), a["ari_reference_inliers"], steps))
                    print(f"raw file, {route:12s} {name:9s} seed {seed:5d}: {stages['loaded']} -> {stages['after_load_filter']} -> {stages['after_distance_error']} rows "
                          f"({int(both.sum())} in common with the reference's): {k} planes, ARI on the reference's inliers {a['ari_reference_inliers']:.3f}, "
                          f"all {a['ari_all']:.3f}, LabelingSteps {steps}", flush=True)
            finally:
                host.mhh_set_data_term(-1)
            summary(f"raw file, {route}, {name}", rows)
    print(flush=True)


def process(sc, H0, hyp, seed=1234):
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((256, 9))
    it, en, secs = C.c_int(0), C.c_double(0), C.c_double(0)
    src, dst, aff, F, e2 = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff, sc.F, sc.e2))
    H0c = None if H0 is None else np.ascontiguousarray(H0)
    t0 = time.perf_counter()
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, F.ctypes.data_as(dp),
                             e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5), 20,
                             C.c_ulonglong(seed), hyp, 32, 20, None if H0c is None else H0c.ctypes.data_as(dp),
                             0 if H0c is None else H0c.shape[0], labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 256, C.byref(it), C.byref(en), C.byref(secs), 0, 4)
    ms = (time.perf_counter() - t0) * 1e3
    return k, labels, it.value, en.value, host.mhh_get_labeling_steps(), ms


def synthetic():
    print("== 2. synthetic scenes with ground truth (seed 1234, 10 planes, post-filter on, at most 20 iterations) ==", flush=True)
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
            for term, name in TERMS:
                host.mhh_set_data_term(term)
                try:
                    k, labels, it, en, steps, _ = process(sc, h0, hyp)
                    times = [process(sc, h0, hyp)[5] for _ in range(REPEAT)] if k >= 0 else [float("nan")]
                finally:
                    host.mhh_set_data_term(-1)
                if k < 0:
                    print(f"{points:6d} {what:24s} {init:30s} {name:9s}: Process() failed", flush=True)
                    continue
                q = mh.synth.agreement(sc.gt_label, labels)
                print(f"{points:6d} {what:24s} {init:30s} {name:9s}: clusters {k:2d}  planes recovered {q['planes_recovered']:2d}/10  ARI {q['ari']:.4f}  "
                      f"iterations {it:2d}  LabelingSteps {steps:2d}  energy {en:.0f}  Process() median of {REPEAT} further calls "
                      f"{statistics.median(times):8.2f} ms (min {min(times):.2f})", flush=True)
    print(flush=True)


def labeling():
    print("== 3. one mh_labeling_step, 50 000 sites x 11 labels, the three labeling scenes of the bench line ==", flush=True)
    for legacy, sep, what in ((False, None, "planes 13 px apart"), (False, 2.0, "planes 2 px apart"), (True, None, "r04 generator")):
        kw = {} if sep is None else {"plane_separation": sep}
        sc = mh.synth.make_scene(50000, 10, seed=1234, legacy_r04=legacy, **kw)
        H = sc.H_true * (1.0 + np.random.default_rng(0).normal(0, 1e-4, size=sc.H_true.shape))
        with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
            e.set_correspondences(sc.src, sc.dst, sc.aff)
            e.set_epipolar(sc.F, sc.e2)
            e.set_neighbors_csr(sc.hit_rowptr, sc.hit_col)
            for _, name in TERMS:
                e.set_data_term(name)
                e.set_models(H)
                e.labeling_step(False, np.full(sc.n, -1, np.int32))           # warm-up
                ts = []
                for _ in range(REPEAT):
                    e.set_models(H)
                    t0 = time.perf_counter()
                    lab, energy, cycles = e.labeling_step(False, np.full(sc.n, -1, np.int32))
                    ts.append((time.perf_counter() - t0) * 1e3)
                st = e.expand_stats()
                q = mh.synth.agreement(sc.gt_label, lab)
                print(f"{what:20s} {name:9s}: energy {int(energy):9d}  cycles {cycles}  moves_run {int(st['moves_run']):3d}  moves_solved {int(st['moves_solved']):3d}  "
                      f"core_max {int(st['core_max']):6d}  planes recovered {q['planes_recovered']:2d}/10  ARI {q['ari']:.4f}  "
                      f"median of {REPEAT} {statistics.median(ts):7.3f} ms (min {min(ts):.3f})", flush=True)
            e.set_data_term("reference")
    print(flush=True)


def cost_matrix():
    print("== 4. mh_cost_matrix, 50 000 points x 100 000 DLT hypotheses (kernel time, mh_profile_get) ==", flush=True)
    sc = mh.synth.make_scene(50000, 10, seed=1234, with_neighbours=False)
    with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
        e.set_correspondences(sc.src, sc.dst, sc.aff)
        e.propose_dlt4(1234, 0, 100000)
        for name in ("reference", "rising", "reference", "rising"):
            e.set_data_term(name)
            e.cost_matrix(fetch_C=False, fetch_counts=False)
            e.synchronize()
            ts = []
            for _ in range(REPEAT):
                e.profile_reset()
                e.profile_enable(True)
                e.cost_matrix(fetch_C=False, fetch_counts=False)
                e.synchronize()
                n, ms = e.profile_get(mh.capi.K_COSTMATRIX)
                e.profile_enable(False)
                ts.append(ms / max(n, 1))
            print(f"{name:9s}: median of {REPEAT} launches {statistics.median(ts):.4f} ms (min {min(ts):.4f}, max {max(ts):.4f})", flush=True)
        e.set_data_term("reference")
    print(flush=True)


if "1" in PARTS:
    barrsmith()
if "2" in PARTS:
    synthetic()
if "3" in PARTS:
    labeling()
if "4" in PARTS:
    cost_matrix()
