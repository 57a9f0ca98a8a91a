"""The minimal-sample F estimator (MultiH::SetFundamentalEstimator(FUND_ESTIMATOR_MINIMAL7), multih_harness --f-estimator
minimal) on the raw barrsmith file, beside the default 8-point route: rows kept after the load filter and after Process()'s
stages, planes and agreement with the reference's labels over the twelve seeds of profiles/r06_barrsmith_agreement.txt,
under both error definitions, and the wall time of one estimate on the raw rows.  Measurement only: nothing here is
asserted by a test.  Needs a GPU.

    python tools/fund7_barrsmith.py [out.txt]
"""
import ctypes as C
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("barrsmith_agreement", os.path.join(ROOT, "tools", "barrsmith_agreement.py"))
B = importlib.util.module_from_spec(spec)
spec.loader.exec_module(B)
mh = B.mh

SEEDS = (1234, 7, 99, 1, 2, 3, 4, 5, 6, 8, 9, 10)
MAX_SAMPLES, CONFIDENCE = 1000, 0.99


def minimal_route(pts, seed, metric, load_filter=2.0, hypotheses=20000):
    """tools/barrsmith_agreement.harness_route with the minimal estimator in both F estimations."""
    host = B._host()
    host.mhh_set_fundamental_estimator.argtypes = [C.c_int, C.c_int, C.c_double]
    host.mhh_set_fundamental_estimator.restype = None
    dp = C.POINTER(C.c_double)
    n0 = len(pts)
    src, dst = (np.ascontiguousarray(pts[:, a:b]) for a, b in ((0, 2), (2, 4)))
    mask = np.ones(n0, dtype=np.uint8)
    host.mhh_set_fundamental_estimator(1, MAX_SAMPLES, CONFIDENCE)
    try:
        k0 = host.mhh_filter_correspondences(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), n0, C.c_double(load_filter),
                                             C.c_ulonglong(seed ^ 0x10adf117e4), 4000, int(metric), 0, mask.ctypes.data_as(C.POINTER(C.c_ubyte)))
        assert k0 >= 8, "the load filter failed"
        rows1 = np.flatnonzero(mask)
        sub = np.ascontiguousarray(pts[rows1])
        e = mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20)
        e.set_fundamental_metric(metric)
        e.set_correspondences(sub[:, 0:2], sub[:, 2:4], sub[:, 4:8])
        F, e2, m, inl, used = e.estimate_fundamental_minimal(seed ^ 0xf00d, MAX_SAMPLES, CONFIDENCE, 2.6)
        e1, e2b = e.epipoles(F)
        keep, _ = e.refine_correspondences(F, e1, e2b, m)
        e.close()
        rows2 = rows1[np.flatnonzero(keep)]
        host.mhh_set_neighbourhood(0, C.c_double(0.0))
        host.mhh_set_neighbourhood_approx(0, 32, C.c_ulonglong(0))
        host.mhh_set_post_filter(1)
        host.mhh_set_fundamental_metric(int(metric))
        s2, d2, a2 = (np.ascontiguousarray(sub[:, a:b]) for a, b in ((0, 2), (2, 4), (4, 8)))
        labels = np.full(len(sub), -7, dtype=np.int32)
        Hout = np.zeros((256, 9))
        it, en = C.c_int(0), C.c_double(0)
        k = host.mhh_run_process(s2.ctypes.data_as(dp), d2.ctypes.data_as(dp), a2.ctypes.data_as(dp), len(sub), None, None,
                                 C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(seed), hypotheses, 32, 0,
                                 None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)), Hout.ctypes.data_as(dp), 256, C.byref(it), C.byref(en),
                                 None, 0, 4)
    finally:
        host.mhh_set_fundamental_estimator(-1, 0, 0.0)
        host.mhh_set_fundamental_metric(-1)
    st = (C.c_int * 4)()
    host.mhh_get_front_stages(st)
    C.CDLL(None).fflush(None)
    stages = {"loaded": int(n0), "after_load_filter": int(len(rows1)), "in_ransac_mask": int(st[1]),
              "after_optimal_triangulation": int(st[2]), "after_distance_error": int(st[3]), "samples_used": int(used)}
    assert st[3] == len(rows2), "the class and its decomposition keep different rows"
    return rows2, labels[:len(rows2)].copy(), int(k), stages


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    pts, ref_rows, ref_labels = B.kept_correspondences(with_rows=True)
    for metric in (1, 0):
        tag = "point-to-line distance" if metric else "Sampson distance"
        for name in ("minimal", "ls8"):
            aris, planes, kept1, kept2 = [], [], [], []
            for seed in SEEDS:
                if name == "minimal":
                    rows, labels, k, st = minimal_route(pts, seed, metric)
                else:
                    rows, labels, k, st = B.harness_route(pts, "dlt", seed, load_filter=2.0, metric=metric)
                full = np.full(len(pts), -2)
                full[rows] = labels
                ours = full[ref_rows]
                both = ours > -2
                a = B.agreement(ours[both], ref_labels[both])
                aris.append(a["ari_reference_inliers"]); planes.append(k)
                kept1.append(st["after_load_filter"]); kept2.append(st["after_distance_error"])
                extra = f", samples used in Process() {st['samples_used']}" if name == "minimal" else ""
                say(f"raw input [load filter 2 px, {tag}], f-estimator {name:7s} seed {seed:5d}: {st['loaded']} -> {st['after_load_filter']} -> "
                    f"{st['in_ransac_mask']} -> {st['after_optimal_triangulation']} -> {st['after_distance_error']} (the reference kept 1094, "
                    f"{int(both.sum())} in common): {k} planes, ARI on the reference's inliers {a['ari_reference_inliers']:.3f}{extra}")
            say(f"   => {name}, {tag}: after the load filter {min(kept1)}-{max(kept1)}, after Process()'s stages {min(kept2)}-{max(kept2)}, "
                f"planes {planes}, median ARI on the reference's inliers {np.median(aris):.3f}, min {min(aris):.3f}, max {max(aris):.3f}")
    # wall time of one estimate on the raw rows (host clock around calls that end in a synchronise), after a warm-up
    e = mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20)
    e.set_fundamental_metric(1)
    e.set_correspondences(pts[:, 0:2], pts[:, 2:4], pts[:, 4:8])
    reps = 50
    for name, call in (("mh_estimate_fundamental, 4000 hypotheses", lambda s: e.estimate_fundamental(s, 4000, 2.0)),
                       ("mh_estimate_fundamental_minimal, 1000 samples, c = 0.99", lambda s: e.estimate_fundamental_minimal(s, MAX_SAMPLES, CONFIDENCE, 2.0))):
        for s in range(5):
            call(1000 + s)
        t = []
        for s in range(reps):
            t0 = time.perf_counter()
            call(s)
            t.append(time.perf_counter() - t0)
        t = np.array(t) * 1e3
        say(f"wall time on the {len(pts)} raw rows, 2.0 px, point-to-line distance: {name}: median {np.median(t):.3f} ms, min {t.min():.3f}, max {t.max():.3f} ({reps} calls)")
    e.close()


if __name__ == "__main__":
    main()
