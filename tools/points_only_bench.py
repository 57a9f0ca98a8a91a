#!/usr/bin/env python3
"""The point-only route on the GPU: the 3-point re-estimator (mh_set_estimator(MH_ESTIMATOR_3PT): member compaction +
k_3pt_reestimate) next to the HAF one (k_haf_reestimate) at 50 000 points x 11 labels and 20 000 points x 540 labels, and
MultiH::Process() by the point-only route next to the route with affinities on the configs[4]-sized scene (50 000 points,
10 planes), with F given and with F estimated.  Every figure is the median of REPS runs (default 21); the re-estimators are
timed by the engine's per-kernel events (mh_profile_*), Process() by the wall clock of a C++ driver
(tools/points_only_process.cpp, built here with g++ against the in-tree libraries), which also runs the route with affinities
and the 3-point refits and reports each route's stage table, labeling steps and loop time.  MH_LIB=multi-h_amd/libmultih_hip_tuning.so
(`python multi-h_amd/build.py --tuning`) adds both forms of the 3-point fit forced (mh_set_tuning key 34: 1 the match loop, 2 the compacted lists).  Prints one JSON line."""
import importlib, json, os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mh = importlib.import_module("multi-h_amd")
REPS = int(os.environ.get("REPS", 21))
K_REESTIMATE = 5


def reestimate_ms(n, nh, estimator, form=0):
    sc = mh.synth.make_scene(n, 10, seed=1234, with_neighbours=False)
    rng = np.random.default_rng(7)
    lab = np.where(sc.gt_label >= 0, sc.gt_label, rng.integers(-1, nh, size=n)).astype(np.int32)
    H0 = np.tile(sc.H_true, ((nh + 9) // 10, 1))[:nh]
    with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
        e.set_correspondences(sc.src, sc.dst, sc.aff)
        e.set_epipolar(sc.F, sc.e2)
        e.set_estimator(estimator)
        if form:
            e.set_tuning(34, form)           # the 3-point fit's match-loop form: measurement libraries only (MH_LIB)
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
    return float(np.median(out))


def process_ms(tmp):
    sc = mh.synth.make_scene(50000, 10, seed=1234, with_neighbours=False)
    corr = os.path.join(tmp, "corr.txt")
    np.savetxt(corr, np.concatenate([sc.src, sc.dst, sc.aff], axis=1), fmt="%.17g")
    epi = os.path.join(tmp, "epi.txt")
    np.savetxt(epi, np.concatenate([sc.F, sc.e2])[None], fmt="%.17g")
    exe = os.path.join(tmp, "points_only_process")
    host = os.path.join(ROOT, "multi-h_amd", "host")
    lib = os.path.join(ROOT, "multi-h_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "points_only_process.cpp"), "-o", exe, "-L" + lib, "-lmultih_host",
                           "-lmultih_hip", "-Wl,-rpath," + lib])
    res = {}
    for tag, extra in (("F_given", [epi]), ("F_estimated", [])):
        p = subprocess.run([exe, corr, str(REPS + 1), *extra], capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise RuntimeError(p.stdout[-2000:] + p.stderr[-2000:])
        rows = [l.split() for l in p.stdout.splitlines() if l.split() and l.split()[0] in ("affine", "affine3pt", "points")]
        for route in ("affine", "affine3pt", "points"):
            t = [float(r[2]) for r in rows if r[0] == route and int(r[1]) >= 1]
            last = [r for r in rows if r[0] == route][-1]
            res[f"process_ms_{route}_{tag}"] = float(np.median(t))
            res[f"clusters_{route}_{tag}"] = int(last[3])
            res[f"labeling_steps_{route}_{tag}"] = int(last[4])
            res[f"loop_ms_{route}_{tag}"] = float(np.median([float(r[5]) for r in rows if r[0] == route and int(r[1]) >= 1]))
            res[f"stages_{route}_{tag}"] = [int(v) for v in last[6:9]]
    return res


out = {"reps": REPS}
for n, nh in ((50000, 11), (20000, 540)):
    for est in ("haf", "3pt"):
        out[f"reestimate_us_{est}_{n}x{nh}"] = round(1e3 * reestimate_ms(n, nh, est), 1)
    if os.environ.get("MH_LIB"):                 # the measurement library also carries the other form of the 3-point fit
        out[f"reestimate_us_3pt_matchloop_{n}x{nh}"] = round(1e3 * reestimate_ms(n, nh, "3pt", form=1), 1)
        out[f"reestimate_us_3pt_compacted_{n}x{nh}"] = round(1e3 * reestimate_ms(n, nh, "3pt", form=2), 1)
if os.environ.get("PROCESS", "1") == "1":
    with tempfile.TemporaryDirectory() as tmp:
        out.update(process_ms(tmp))
print(json.dumps(out))
