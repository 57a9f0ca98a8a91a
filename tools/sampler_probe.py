#!/usr/bin/env python3
"""What the neighbourhood-guided proposal sampler (MultiH::SetProposalSampler, mh_set_sampler) buys on the whole route, on an
MI355X: Process() of the host class by the default route (DLT proposals + greedy selection, then the loop), F given, on

  50 000 points / 10 planes (the configs[4]-sized scene of bench.py full_loop), 20 000 / 6 and 5 000 / 3   (seed 1234)

once with the uniform sampler at the route's hypothesis count M (2 hypotheses per point: 100 000 at configs[4]) and with the
local sampler at M, M/4 and M/10 for k in {16, 32} and uniform_per_16 in {0, 4, 8}.  Per run: planes recovered and ARI against
the generator's ground truth (synth.agreement), the median wall time of REPEAT (20) further calls in the same process, the
time of the table build (mh_build_sample_neighbours, median of 5), and — once, at 50 000 points — the kernel time of
100 000 hypotheses under either sampler in either form of the proposer (mh_profile_get(MH_K_DLT4)).

  python tools/sampler_probe.py > profiles/sampler_probe.txt
Env: REPEAT (20), SCENES ("50000:10,20000:6,5000:3")."""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mh = importlib.import_module("multi-h_amd")
REPEAT = int(os.environ.get("REPEAT", 20))
SCENES = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("SCENES", "50000:10,20000:6,5000:3").split(",")]
host = C.CDLL(os.path.join(ROOT, "multi-h_amd", "libmultih_host.so"))
dp = C.POINTER(C.c_double)


def process(sc, hyp):
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((256, 9))
    it, en, secs = C.c_int(0), C.c_double(0), C.c_double(0)
    src, dst, aff, F, e2 = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff, sc.F, sc.e2))
    t0 = time.perf_counter()
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, F.ctypes.data_as(dp),
                             e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5), 20,
                             C.c_ulonglong(1234), hyp, 32, 20, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 256, C.byref(it), C.byref(en), C.byref(secs), 0, 4)
    return k, labels, (time.perf_counter() - t0) * 1e3


def run(sc, planes, hyp, sampler, k=0, u=0):
    host.mhh_set_proposal_sampler(sampler, k, u)
    try:
        clusters, labels, _ = process(sc, hyp)                  # the first call also pays for whatever the process has not loaded yet
        if clusters < 0:
            return f"{'local' if sampler else 'uniform':8s} k {k:2d} u {u:2d} hypotheses {hyp:6d}: Process() failed"
        times = [process(sc, hyp)[2] for _ in range(REPEAT)]
    finally:
        host.mhh_set_proposal_sampler(0, 0, 0)
    q = mh.synth.agreement(sc.gt_label, labels)
    return (f"{'local' if sampler else 'uniform':8s} k {k:2d} u {u:2d} hypotheses {hyp:6d}: clusters {clusters:2d}  planes recovered "
            f"{q['planes_recovered']:2d}/{planes}  ARI {q['ari']:.4f}  Process() median of {REPEAT} further calls {statistics.median(times):8.2f} ms "
            f"(min {min(times):.2f})")


def table_build_ms(sc, k):
    with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
        e.set_correspondences(sc.src, sc.dst, sc.aff)
        e.build_sample_neighbours(k)
        ts = []
        for _ in range(5):
            e.synchronize()
            t0 = time.perf_counter()
            e.build_sample_neighbours(k)                        # (synchronises: it reads the error word back)
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def kernel_figures(sc, m=100000, reps=20):
    print(f"k_dlt4 per {m} hypotheses at {sc.n} points, mean of {reps} launches (mh_profile_get(MH_K_DLT4)), one process, this box:")
    with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
        e.set_correspondences(sc.src, sc.dst, sc.aff)
        e.build_sample_neighbours(32)
        for form, name in ((2, "register form (mh_propose_dlt4)"), (1, "LDS-staged form (mh_prefetch_dlt4)")):
            e.set_tuning(25, form)
            for sampler, u, what in ((0, 0, "uniform"), (1, 0, "local k 32 u 0"), (1, 4, "local k 32 u 4"), (0, 0, "uniform again")):
                e.set_sampler(sampler, u)
                e.propose_dlt4(1234, 0, m)
                e.synchronize()
                e.profile_reset()
                e.profile_enable(True)
                for r in range(reps):
                    e.propose_dlt4(1234, r * m, m)
                e.synchronize()
                n, ms = e.profile_get(mh.capi.K_DLT4)
                e.profile_enable(False)
                print(f"  {name:36s} {what:16s} {ms / max(n, 1):.4f} ms")
        e.set_tuning(25, 0)


for points, planes in SCENES:
    sc = mh.synth.make_scene(points, planes, seed=1234, with_neighbours=False)
    M = 2 * points
    print(f"== {points} points / {planes} planes, M = {M} ==", flush=True)
    for k in (16, 32):
        print(f"table build (mh_build_sample_neighbours, k = {k}): {table_build_ms(sc, k):.3f} ms")
    print(run(sc, planes, M, 0), flush=True)
    for hyp in (M, M // 4, M // 10):
        for k in (16, 32):
            for u in (0, 4, 8):
                print(run(sc, planes, hyp, 1, k, u), flush=True)
    if points == 50000:
        kernel_figures(sc)
    print(flush=True)
