#!/usr/bin/env python3
"""What the 3-point proposals (mh_propose_3pt, csrc/propose3pt.hip; MultiH::PROPOSAL_SOURCE_3PT) cost and buy, on one MI355X:

  kernel     mh_propose_3pt at 100 000 hypotheses / 50 000 correspondences under the uniform and the local sampler (k = 32,
             4 of 16 uniform), mh_propose_dlt4 beside each, interleaved in one process: wall time of the call + synchronize,
             median of 20 with min and max.
  default    Process() by the DEFAULT route, F given, on 50 000 / 10, 20 000 / 6 and 5 000 / 3 (seed 1234): this tree's libraries
             against another build's (--parent DIR: the multi-h_amd directory of a build of the parent commit), child processes
             in the order parent / this / parent, each: one warm-up call, then 20 calls, median with min and max.  Without
             --parent only this tree is measured.
  route      the same scenes, F given, the default route at M = 2 n hypotheses against the 3-point source at M, M/4 and M/10:
             with affinities (mhh_run_process) and point-only (multih_harness --points --epipolar).  Planes recovered, ARI, loop
             iterations, models handed to the loop (the 3-point route's log line), clusters after the first MergingStep (the stage
             log's "iteration 1" line), ms per Process() (with affinities: second call / median of five more; point-only: the
             last stage line of one harness run).
  barrsmith  the raw barrsmith file through the harness route of tools/barrsmith_agreement.py (load filter 2 px, point-to-line
             distance), the twelve seeds of profiles/r06_barrsmith_agreement.txt: the default route against the 3-point source.

  python tools/propose_3pt_probe.py [--parent DIR] | grep -v '^\\[Multi-H\\]' > profiles/propose_3pt_probe.txt
Without a part as argument the parts run one after the other, each as a child process under a time limit of its own, the next
only if the one before ended well."""
import ctypes as C
import importlib
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIMITS = {"kernel": 120, "default": 240, "route": 300, "barrsmith": 240}            # seconds
SEEDS12 = (1234, 7, 99, 1, 2, 3, 4, 5, 6, 8, 9, 10)
SCENES = ((50000, 10), (20000, 6), (5000, 3))
PKG = os.path.join(ROOT, "multi-h_amd")
STAGE = re.compile(r"\[Multi-H\] (.+) done ([0-9.]+) ms after Process\(\) began")
HANDED = re.compile(r"\[Multi-H\] Proposed (\d+) models from (\d+) 3PT hypotheses")
FIRST_MERGE = re.compile(r"\[Multi-H\] iteration 1: (\d+) clusters")


def _host(pkg=PKG):
    return C.CDLL(os.path.join(pkg, "libmultih_host.so"))


def _timed(e, call, reps=20):
    call()
    e.synchronize()
    ts = []
    for _ in range(reps):
        e.synchronize()
        t0 = time.perf_counter()
        call()
        e.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def kernel():
    mh = importlib.import_module("multi-h_amd")
    n, m = 50000, 100000
    sc = mh.synth.make_scene(n, 10, seed=1234, with_neighbours=False)
    print(f"== {m} hypotheses over {n} correspondences (wall time of call + synchronize, median of 20 (min, max)) ==", flush=True)
    with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
        e.set_correspondences(sc.src, sc.dst, sc.aff)
        e.set_epipolar(sc.F, sc.e2)
        for sampler in ("uniform", "local (k = 32, 4 of 16 uniform)"):
            if sampler != "uniform":
                e.build_sample_neighbours(32)
                e.set_sampler(1, 4)
            for rnd in range(2):                                   # interleaved: DLT, 3-point, DLT, 3-point
                print(f"{sampler:32s} mh_propose_dlt4 : %.3f ms (%.3f, %.3f)" % _timed(e, lambda: e.propose_dlt4(1234, 0, m)), flush=True)
                print(f"{sampler:32s} mh_propose_3pt  : %.3f ms (%.3f, %.3f)" % _timed(e, lambda: e.propose_3pt(1234, 0, m)), flush=True)
            H = e.get_models()
            print(f"    3-point fits that failed (all-NaN rows): {int(np.isnan(H).all(axis=1).sum())} of {m}", flush=True)


def _process(host, sc, hyp, seed=1234):
    dp = C.POINTER(C.c_double)
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((256, 9))
    it, en, secs = C.c_int(0), C.c_double(0), C.c_double(0)
    src, dst, aff, F, e2 = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff, sc.F, sc.e2))
    t0 = time.perf_counter()
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n, F.ctypes.data_as(dp),
                             e2.ctypes.data_as(dp), C.c_double(2.6), C.c_double(2.2), C.c_double(0.005), C.c_double(0.5), 20,
                             C.c_ulonglong(seed), hyp, 32, 20, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)),
                             Hout.ctypes.data_as(dp), 256, C.byref(it), C.byref(en), C.byref(secs), 0, 4)
    return k, labels, (time.perf_counter() - t0) * 1e3, it.value


def default_child(pkg, tag):
    """One process of the parent / this / parent comparison: the default route through the libraries under `pkg`."""
    mh = importlib.import_module("multi-h_amd")
    host = _host(pkg)
    for points, planes in SCENES:
        sc = mh.synth.make_scene(points, planes, seed=1234, with_neighbours=False)
        runs = [_process(host, sc, 2 * points) for _ in range(21)]
        ms = [r[2] for r in runs[1:]]
        q = mh.synth.agreement(sc.gt_label, runs[0][1])
        print(f"{tag:6s} {points:6d} / {planes:2d}: clusters {runs[0][0]:2d}, planes {q['planes_recovered']}/{planes}, ARI {q['ari']:.4f}; "
              f"median of 20 calls {statistics.median(ms):.2f} ms (min {min(ms):.2f}, max {max(ms):.2f})", flush=True)


def default(parent):
    print("== Process(), DEFAULT route, F given, seed 1234, 2 n DLT hypotheses: one process after the other ==", flush=True)
    order = [("parent", parent), ("this", PKG), ("parent", parent)] if parent else [("this", PKG)]
    if not parent:
        print("(no --parent build given: this tree alone)", flush=True)
    for tag, pkg in order:
        r = subprocess.run(["timeout", "-k", "10", "70", sys.executable, os.path.abspath(__file__), "default_child", pkg, tag])
        if r.returncode != 0:
            sys.exit(r.returncode)


def _configs(points):
    M = 2 * points
    return ((0, M), (2, M), (2, M // 4), (2, M // 10))            # (source, hypotheses)


def route_child():
    """With affinities: every configuration seven times in this process; the second call's stage log goes between @@ marks."""
    mh = importlib.import_module("multi-h_amd")
    host = _host()
    libc = C.CDLL(None)
    for points, planes in SCENES:
        sc = mh.synth.make_scene(points, planes, seed=1234, with_neighbours=False)
        for source, hyp in _configs(points):
            host.mhh_set_proposal_source(source, 0, 1)
            try:
                runs = []
                for i in range(7):
                    if i == 1:
                        print(f"@@ {points} {planes} {source} {hyp}", flush=True)
                    runs.append(_process(host, sc, hyp))
                    libc.fflush(None)
                    if i == 1:
                        print("@@ end", flush=True)
            finally:
                host.mhh_set_proposal_source(0, 16, 1)
            k, labels, _, it = runs[1]
            if min(r[0] for r in runs) < 0:                        # a Process() that failed: nothing more is started on the card
                print(f"{points} / {planes}, source {source}, {hyp} hypotheses: Process() failed", flush=True)
                sys.exit(1)
            q = mh.synth.agreement(sc.gt_label, labels)
            ms = [r[2] for r in runs]
            print(f"@@ result clusters {k} planes {q['planes_recovered']} ari {q['ari']:.4f} it {it} "
                  f"second {ms[1]:.2f} median {statistics.median(ms[2:]):.2f}", flush=True)


def _name(source):
    return "default (DLT)" if source == 0 else "3-point      "


def _points_only(mh):
    """Point-only: one harness run per configuration (F given through --epipolar), its stage log and its result file."""
    harness = os.path.join(PKG, "multih_harness")
    env = dict(os.environ, MULTIH_TIMING="1")
    with tempfile.TemporaryDirectory() as tmp:
        for points, planes in SCENES:
            sc = mh.synth.make_scene(points, planes, seed=1234, with_neighbours=False)
            corr, epi = os.path.join(tmp, "corr.txt"), os.path.join(tmp, "epi.txt")
            np.savetxt(corr, np.concatenate([sc.src, sc.dst], axis=1), fmt="%.17g")
            np.savetxt(epi, np.concatenate([np.ravel(sc.F), np.ravel(sc.e2)])[None, :], fmt="%.17g")
            for source, hyp in _configs(points):
                out = os.path.join(tmp, "out.txt")
                cmd = ["timeout", "-k", "10", "60", harness, corr, out, "--points", "--epipolar", epi, "--hypotheses", str(hyp), "--seed", "1234",
                       "--thrH", "2.2"] + (["--proposals", "3pt"] if source else [])
                r = subprocess.run(cmd, capture_output=True, text=True, env=env)
                if r.returncode != 0:                              # nothing more is started on the card after a run that failed
                    print(f"{points:6d} / {planes:2d} point-only {_name(source)} {hyp:6d} hypotheses: exit status {r.returncode}: {r.stderr[-300:]}", flush=True)
                    sys.exit(r.returncode)
                res = np.loadtxt(out, ndmin=2)
                full = np.full(sc.n, -1, dtype=np.int64)
                if res.shape[0] == sc.n:
                    full[:] = res[:, 4]
                else:
                    for a in range(0, res.shape[0], 256):
                        d = ((res[a:a + 256, None, :2] - sc.src[None, :, :]) ** 2).sum(-1)
                        full[np.argmin(d, axis=1)] = res[a:a + 256, 4]
                q = mh.synth.agreement(sc.gt_label, full)
                stages = [(m.group(1), float(m.group(2))) for m in map(STAGE.match, r.stdout.splitlines()) if m]
                handed = HANDED.search(r.stdout)
                merged = FIRST_MERGE.search(r.stdout)
                its = len(re.findall(r"\[Multi-H\] iteration \d+:", r.stdout))
                print(f"{points:6d} / {planes:2d} point-only {_name(source)}: hypotheses {hyp:6d}, planes {q['planes_recovered']}/{planes}, ARI {q['ari']:.4f}, "
                      f"loop iterations {its}, handed to the loop {handed.group(1) if handed else '-'}, after the first MergingStep "
                      f"{merged.group(1) if merged else '-'}, last stage {stages[-1][0] if stages else '-'} at {stages[-1][1] if stages else float('nan'):.2f} ms", flush=True)


def route():
    print("== Process(), F given, seed 1234: the default route (2 n DLT hypotheses) and the 3-point source at M, M/4, M/10 ==", flush=True)
    env = dict(os.environ, MULTIH_TIMING="1")
    r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "route_child"], env=env,
                       capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stdout[-3000:] + r.stderr[-3000:], flush=True)
        sys.exit(r.returncode)
    cur, log = None, []
    for line in r.stdout.splitlines():
        if line.startswith("@@ end"):
            pass
        elif line.startswith("@@ result"):
            f = line.split()
            text = "\n".join(log)
            names = [(m.group(1), float(m.group(2))) for m in map(STAGE.match, log) if m]
            idx = [s for s, _ in names].index("initial models") if "initial models" in [s for s, _ in names] else -1
            init = names[idx][1] - names[idx - 1][1] if idx > 0 else float("nan")
            handed, merged = HANDED.search(text), FIRST_MERGE.search(text)
            points, planes, source, hyp = cur
            print(f"{points:6d} / {planes:2d} affinities {_name(source)}: hypotheses {hyp:6d}, clusters {f[3]:>2s}, planes {f[5]}/{planes}, ARI {f[7]}, "
                  f"loop iterations {f[9]}, handed to the loop {handed.group(1) if handed else '-'}, after the first MergingStep "
                  f"{merged.group(1) if merged else '-'}, initial models {init:.2f} ms, Process() second call {f[11]} ms / median of five more {f[13]} ms", flush=True)
        elif line.startswith("@@ "):
            cur, log = tuple(int(v) for v in line.split()[1:]), []
        else:
            log.append(line)
    _points_only(importlib.import_module("multi-h_amd"))


def barrsmith():
    B = importlib.import_module("barrsmith_agreement")
    host = _host()
    pts, ref_rows, ref_labels = B.kept_correspondences(with_rows=True)
    print("== raw barrsmith file, harness route (load filter 2 px, point-to-line distance), twelve seeds ==", flush=True)
    res = {}
    for source, name in ((0, "default (DLT)"), (2, "3-point")):
        res[name] = []
        for seed in SEEDS12:
            host.mhh_set_proposal_source(source, 0, 1)
            try:
                t0 = time.perf_counter()
                rows, labels, k, _ = B.harness_route(pts, "dlt", seed, 2.0, 1)
                ms = (time.perf_counter() - t0) * 1e3
            finally:
                host.mhh_set_proposal_source(0, 16, 1)
            full = np.full(len(pts), -2, dtype=int)
            full[rows] = labels
            ours = full[ref_rows]
            both = ours > -2
            ari = B.agreement(ours[both], ref_labels[both])["ari_reference_inliers"] if k > 0 else float("nan")
            res[name].append((k, ari))
            print(f"{name:13s} seed {seed:5d}: {k} planes, ARI on the reference's inliers {ari:.3f}, route wall time {ms:.1f} ms", flush=True)
    for name, r in res.items():
        aris = sorted(a for _, a in r)
        print(f"   => {name}: planes {[k for k, _ in r]}, median ARI {statistics.median(aris):.3f}, min {aris[0]:.3f}, max {aris[-1]:.3f}", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    parent = ""
    if "--parent" in args:
        i = args.index("--parent")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    part = args[0] if args else ""
    if part == "default_child":
        default_child(args[1], args[2])
    elif part == "route_child":
        route_child()
    elif part in LIMITS:
        {"kernel": kernel, "default": lambda: default(parent), "route": route, "barrsmith": barrsmith}[part]()
    else:
        for part in LIMITS:
            cmd = ["timeout", "-k", "10", str(LIMITS[part]), sys.executable, os.path.abspath(__file__), part] + (["--parent", parent] if parent else [])
            r = subprocess.run(cmd)
            if r.returncode != 0:
                print(f"{part}: exit status {r.returncode}; the parts after it were not run", flush=True)
                sys.exit(r.returncode)
