#!/usr/bin/env python3
"""What the compatibility check without F (mh_compat_dlt_medians; csrc/dlt4.hip k_dlt4 under the segment sampler, csrc/compat.hip
k_compat_median4 and k_compat_cluster_median; MultiH::SetCompatibilityFit) rests on and costs:

  grid     (no GPU) the twin tests/compat_dlt_numpy.py on clean planes — members x noise x perspective on the whole image, members
           x noise on a third of it, each cell once per draw, 501 trials: the ratio statistic / sigma^2, its largest value and A,
           that value rounded up to a power of two (the default limit scale); then the contaminated counter-cases against
           A thr_hom^2.
  call     one MI355X: time per mh_compat_dlt_medians call, copies included (host clock around the call, which ends in a stream
           synchronise), the median of REPS calls (default 21) behind two that are left out, at 50 000 points / 11 clusters and at
           20 000 points / 540 clusters, 501 trials; the same calls split by launch with the engine's events (mh_profile_*: the
           fits in the MH_K_DLT4 slot, the trial values in MH_K_SCORE, the cluster values in MH_K_REESTIMATE); and beside them the
           3-point check on the same labelled scenes (multih::CompatibilityCheck with mh_compat_trial_stats_fit plus the host's
           replay and bookkeeping, through mhh_compatibility_medians_on_engine), same session.
  process  Process() on the three-motion scene (1 200 points) without epipolar geometry, with the check off and with the 4-point
           check: clusters, planes recovered, wall time of the call (median of 5 behind one).

  python tools/compat_dlt_probe.py | grep -v '^\\[Multi-H\\]\\|^Iteration' > profiles/compat_dlt_probe.txt
Every part is a child process under a time limit of its own; nothing more is started after a part that did not end well."""
import ctypes as C
import importlib
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LIMIT = 240                                        # seconds per part
REPS = int(os.environ.get("REPS", 21))
THR = 2.2
TRIALS = 501
K_DLT4, K_SCORE, K_REESTIMATE = 0, 2, 5
SEEDS = (1234, 7, 99, 1, 2, 3, 4, 5, 6, 8, 9, 10)
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def grid():
    import compat_dlt_numpy as T
    rows = T.clean_grid()
    print(f"== clean planes, {T.GRID_TRIALS} trials, draws {T.GRID_DRAWS}: statistic / sigma^2, min .. max over the draws ==")
    for third in (False, True):
        for p in (T.GRID_PERSPECTIVE if not third else T.GRID_PERSPECTIVE[1:2]):
            print(f"  {'a third of the image' if third else 'the whole image'}, perspective {p:g}")
            for n in T.GRID_MEMBERS:
                cells = []
                for s in T.GRID_SIGMA:
                    v = [r[5] for r in rows if r[0] == n and r[1] == s and r[2] == p and r[3] == third]
                    cells.append(f"sigma {s}: {min(v):6.1f} .. {max(v):6.1f}")
                print(f"    {n:5d} members   " + "   ".join(cells))
    ratios = np.array([r[5] for r in rows])
    whole = np.array([r[5] for r in rows if not r[3]])
    print(f"  whole image: median {np.median(whole):.1f}, max {whole.max():.1f}; all {len(rows)} cells: max {ratios.max():.1f} at "
          f"{rows[int(ratios.argmax())][:5]}")
    print(f"  A = {T.LIMIT_SCALE:g} (the next power of two); limit at thr_hom = {THR}: {T.LIMIT_SCALE * THR * THR:.0f} px^2")
    print("== contaminated 400-member clusters, sigma 0.5 ==")
    for name, stat in T.contaminated_grid():
        print(f"  {name:20s} {stat:12.4g} px^2 = {stat / (T.LIMIT_SCALE * THR * THR):7.1f} x the limit")


def _scenes(mh):
    """(name, scene, labels, nh): 50 000 points / 11 clusters (the ten planes and one cluster of outliers) and 20 000 / 540 (the
    planes' points cut into 540 runs)."""
    sc = mh.synth.make_scene(50000, 10, seed=1234, with_neighbours=False)
    lab = np.where(sc.gt_label >= 0, sc.gt_label, 10).astype(np.int32)
    yield "50 000 points / 11 clusters", sc, lab, 11
    sc = mh.synth.make_scene(20000, 10, seed=1234, with_neighbours=False)
    order = np.argsort(np.where(sc.gt_label >= 0, sc.gt_label, 10), kind="stable")
    lab = np.empty(sc.n, dtype=np.int32)
    lab[order] = (np.arange(sc.n) * 540) // sc.n
    yield "20 000 points / 540 clusters", sc, lab, 540


def call():
    mh = importlib.import_module("multi-h_amd")
    import compat_dlt_numpy as T
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    print(f"== per call, median of {REPS} behind 2 (ms): mh_compat_dlt_medians with {TRIALS} trials, copies included; its three "
          "launches by the engine's events; the 3-point check on the same clusters ==", flush=True)
    for name, sc, lab, nh in _scenes(mh):
        pts, begin = T.pack(sc.src, sc.dst, lab, range(nh))
        H0 = np.tile(sc.H_true, ((nh + 9) // 10, 1))[:nh]
        src, dst, F = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.F))
        with mh.Engine(0, 2.6, THR, 0.005, 0.5, 20) as e:
            wall, parts = [], []
            e.profile_enable(True)
            for r in range(REPS + 2):
                e.profile_reset()
                t0 = time.perf_counter()
                med = e.compat_dlt_medians(pts, begin, 4242, 0, TRIALS)[0]
                t1 = time.perf_counter()
                e.synchronize()
                if r >= 2:
                    wall.append(1e3 * (t1 - t0))
                    parts.append([e.profile_get(k)[1] for k in (K_DLT4, K_SCORE, K_REESTIMATE)])
            e.profile_enable(False)
            plain = []
            for r in range(REPS + 2):                                       # (without the events and the optional outputs)
                t0 = time.perf_counter()
                rc = e.lib.mh_compat_dlt_medians(e._h, pts.ctypes.data_as(_dp), begin.ctypes.data_as(_ip), nh, C.c_ulonglong(4242),
                                                 C.c_longlong(0), TRIALS, med.ctypes.data_as(_dp), None, None, None)
                t1 = time.perf_counter()
                assert rc == 0
                if r >= 2:
                    plain.append(1e3 * (t1 - t0))
            three = []
            for r in range(REPS + 2):
                H = H0.copy(); l2 = lab.copy(); m3 = np.zeros(nh)
                t0 = time.perf_counter()
                kept = host.mhh_compatibility_medians_on_engine(e._h, src.ctypes.data_as(_dp), dst.ctypes.data_as(_dp), sc.n,
                                                                l2.ctypes.data_as(_ip), H.ctypes.data_as(_dp), nh, F.ctypes.data_as(_dp),
                                                                C.c_double(THR * THR), 20, C.c_ulonglong(4242), m3.ctypes.data_as(_dp))
                t1 = time.perf_counter()
                assert kept >= 0
                if r >= 2:
                    three.append(1e3 * (t1 - t0))
            p = np.median(np.array(parts), axis=0)
            print(f"  {name}: medians only {np.median(plain):.3f}, with every output {np.median(wall):.3f}; launches: fits {p[0]:.3f}, "
                  f"trial values {p[1]:.3f}, cluster values {p[2]:.3f}; 3-point check (engine + host) {np.median(three):.3f}; "
                  f"clusters over the limit {int((med > T.LIMIT_SCALE * THR * THR).sum())} of {nh}", flush=True)


def process():
    mh = importlib.import_module("multi-h_amd")
    import reestimate_dlt_numpy as D
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    host.mhh_set_compat_fit.argtypes, host.mhh_set_compat_fit.restype = [C.c_int, C.c_int, C.c_double], None
    sc = D.three_motions(1200)
    src, dst, aff = (np.ascontiguousarray(v) for v in (sc.src, sc.dst, sc.aff))
    print("== Process() without epipolar geometry, three motions, 1 200 points: wall time of the call, median of 5 behind 1 ==", flush=True)
    host.mhh_set_epipolar_free(1)
    for name, fit in (("the check skipped (COMPAT_FIT_3PT)", 0), ("the 4-point check (COMPAT_FIT_DLT, 501 trials)", 1)):
        host.mhh_set_compat_fit(fit, TRIALS, 0.0)
        times = []
        for r in range(6):
            labels = np.full(sc.n, -7, dtype=np.int32)
            Hout = np.zeros((64, 9))
            it, en = C.c_int(-1), C.c_double(-1)
            t0 = time.perf_counter()
            k = host.mhh_run_process(src.ctypes.data_as(_dp), dst.ctypes.data_as(_dp), aff.ctypes.data_as(_dp), sc.n, None, None,
                                     C.c_double(2.6), C.c_double(THR), C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(5), 4000, 16, 0,
                                     None, 0, labels.ctypes.data_as(_ip), Hout.ctypes.data_as(_dp), 64, C.byref(it), C.byref(en), None, 0, 4)
            t1 = time.perf_counter()
            assert k >= 0
            if r >= 1:
                times.append(1e3 * (t1 - t0))
        C.CDLL(None).fflush(None)
        got = mh.synth.agreement(sc.gt_label, labels)
        print(f"  {name}: {k} clusters, planes {got['planes_recovered']} of {got['planes']}, ARI {got['ari']:.4f}, {np.median(times):.2f} ms",
              flush=True)
    host.mhh_set_compat_fit(0, TRIALS, 0.0)
    host.mhh_set_epipolar_free(0)


def barrsmith():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import barrsmith_agreement as B
    host = B._host()
    host.mhh_set_compat_fit.argtypes, host.mhh_set_compat_fit.restype = [C.c_int, C.c_int, C.c_double], None
    corr, ref, _, _ = B.kept_correspondences()
    src, dst, aff = (np.ascontiguousarray(corr[:, a:b]) for a, b in ((0, 2), (2, 4), (4, 8)))
    n = len(src)
    print(f"== barrsmith, the reference's {n} rows ({int(ref.max()) + 1} planes), no epipolar geometry, 20 000 hypotheses, seeds {SEEDS}: "
          "clusters and the ARI on the reference's inliers ==", flush=True)
    host.mhh_set_neighbourhood(0, C.c_double(0.0))
    host.mhh_set_epipolar_free(1)
    inl = ref >= 0
    rows = {0: [], 1: []}
    for seed in SEEDS:
        for fit in (0, 1):
            host.mhh_set_compat_fit(fit, TRIALS, 0.0)
            labels = np.full(n, -7, dtype=np.int32)
            Hout = np.zeros((256, 9))
            it, en = C.c_int(0), C.c_double(0)
            k = host.mhh_run_process(src.ctypes.data_as(_dp), dst.ctypes.data_as(_dp), aff.ctypes.data_as(_dp), n, None, None, C.c_double(2.6),
                                     C.c_double(THR), C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(seed), 20000, 32, 0, None, 0,
                                     labels.ctypes.data_as(_ip), Hout.ctypes.data_as(_dp), 256, C.byref(it), C.byref(en), None, 0, 4)
            assert k >= 0
            rows[fit].append((k, B.adjusted_rand(labels[inl], ref[inl])))
        C.CDLL(None).fflush(None)
        print(f"  seed {seed:5d}: {rows[0][-1][0]:2d} clusters, ARI {rows[0][-1][1]:.3f}  ->  with the 4-point check {rows[1][-1][0]:2d} clusters, "
              f"ARI {rows[1][-1][1]:.3f}", flush=True)
    host.mhh_set_compat_fit(0, TRIALS, 0.0)
    host.mhh_set_epipolar_free(0)
    for fit, name in ((0, "the check skipped"), (1, "the 4-point check")):
        k = np.array([r[0] for r in rows[fit]]); a = np.array([r[1] for r in rows[fit]])
        print(f"  {name}: clusters {int(k.min())}..{int(k.max())} (median {np.median(k):g}), ARI median {np.median(a):.3f} "
              f"(min {a.min():.3f}, max {a.max():.3f})", flush=True)


PARTS = {"grid": grid, "call": call, "process": process, "barrsmith": barrsmith}

if __name__ == "__main__":
    if len(sys.argv) > 1:
        PARTS[sys.argv[1]]()
        sys.exit(0)
    for part in PARTS:
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), part])
        if r.returncode != 0:
            print(f"part {part} ended with status {r.returncode}: nothing more is started", flush=True)
            sys.exit(1)
