#!/usr/bin/env python3
"""What the HAF proposals (mh_propose_haf, csrc/haf_propose.hip; MultiH::SetProposalSource) cost and buy, on one MI355X:

  kernel     mh_propose_haf at 50 000 correspondences for members 0 / 16 / 32 (stride 1): wall time of the call + synchronize,
             median of 20 with min and max; the table build (mh_build_sample_neighbours, k = 16 / 32) stated separately; and
             mh_propose_dlt4 at 100 000 hypotheses in the same process beside it for scale.
  default    Process() by the DEFAULT route, F given, on 50 000 / 10, 20 000 / 6 and 5 000 / 3 (seed 1234): this tree's libraries
             against another build's (--parent DIR: the multi-h_amd directory of a build of the parent commit), child processes
             in the order parent / this / parent, each: one warm-up call, then 20 calls, median with min and max.  Without
             --parent only this tree is measured.
  haf        the same scenes under HAF proposals, members 0 / 16 x stride 1 / 4, beside the default route: planes recovered, ARI,
             hypotheses, models handed to the loop, the `initial models` stage (MULTIH_TIMING: from the stage before it to
             "initial models done"; the neighbour table has a stage line of its own), loop iterations, ms per Process() (second
             call / median of five more).
  barrsmith  the raw barrsmith file through the harness route of tools/barrsmith_agreement.py (load filter 2 px, point-to-line
             distance), the twelve seeds of profiles/r06_barrsmith_agreement.txt: the default route against HAF (16, 1) and (32, 1).

  python tools/haf_proposal_probe.py [--parent DIR] | grep -v '^\\[Multi-H\\]' > profiles/haf_proposal_probe.txt
Without a part as argument the parts run one after the other, each as a child process under a time limit of its own, the next
only if the one before ended well."""
import ctypes as C
import importlib
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIMITS = {"kernel": 120, "default": 240, "haf": 300, "barrsmith": 300}            # seconds
SEEDS12 = (1234, 7, 99, 1, 2, 3, 4, 5, 6, 8, 9, 10)
SCENES = ((50000, 10), (20000, 6), (5000, 3))
PKG = os.path.join(ROOT, "multi-h_amd")


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
    n, thr2 = 50000, 2.2 * 2.2
    sc = mh.synth.make_scene(n, 10, seed=1234, with_neighbours=False)
    print(f"== mh_propose_haf, {n} correspondences, stride 1, thr2 {thr2:.2f} (wall time of call + synchronize, median of 20 (min, max)) ==", flush=True)
    with mh.Engine(0, 2.6, 2.2, 0.005, 0.5, 20) as e:
        e.set_correspondences(sc.src, sc.dst, sc.aff)
        e.set_epipolar(sc.F, sc.e2)
        print("mh_propose_dlt4, 100 000 hypotheses      : %.3f ms (%.3f, %.3f)" % _timed(e, lambda: e.propose_dlt4(1234, 0, 100000)), flush=True)
        print("mh_propose_haf, members  0               : %.3f ms (%.3f, %.3f)" % _timed(e, lambda: e.propose_haf(0, n, 1, 0, thr2)), flush=True)
        for k in (16, 32):
            print("mh_build_sample_neighbours, k = %2d       : %.3f ms (%.3f, %.3f)" % ((k,) + _timed(e, lambda: e.build_sample_neighbours(k))), flush=True)
            print("mh_propose_haf, members %2d               : %.3f ms (%.3f, %.3f)" % ((k,) + _timed(e, lambda: e.propose_haf(0, n, 1, k, thr2))), flush=True)
            used = e.get_haf_support()
            bits = np.unpackbits(used.view(np.uint8)).sum()
            print(f"    consistent neighbours per hypothesis: mean {bits / n:.2f}, hypotheses with none {int((used == 0).sum())}", flush=True)
        print("mh_propose_haf, members 16, stride 4     : %.3f ms (%.3f, %.3f)" % _timed(e, lambda: e.propose_haf(0, (n + 3) // 4, 4, 16, thr2)), flush=True)


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


def haf_child():
    mh = importlib.import_module("multi-h_amd")
    host = _host()
    libc = C.CDLL(None)
    for points, planes in SCENES:
        sc = mh.synth.make_scene(points, planes, seed=1234, with_neighbours=False)
        for source, members, stride in ((0, 0, 1), (1, 0, 1), (1, 0, 4), (1, 16, 1), (1, 16, 4)):
            host.mhh_set_proposal_source(source, members, stride)
            try:
                runs = []
                for i in range(7):
                    if i == 1:
                        print(f"@@ {points} {planes} {source} {members} {stride}", flush=True)
                    runs.append(_process(host, sc, 2 * points))
                    libc.fflush(None)
                    if i == 1:
                        print("@@ end", flush=True)
            finally:
                host.mhh_set_proposal_source(0, 16, 1)
            k, labels, _, it = runs[1]
            q = mh.synth.agreement(sc.gt_label, labels) if k >= 0 else {"planes_recovered": -1, "ari": float("nan")}
            ms = [r[2] for r in runs]
            print(f"@@ result clusters {k} planes {q['planes_recovered']} ari {q['ari']:.4f} it {it} "
                  f"second {ms[1]:.2f} median {statistics.median(ms[2:]):.2f}", flush=True)


def haf():
    """Runs haf_child with MULTIH_TIMING set and reads the stage lines of each configuration's second call."""
    print("== Process(), F given, seed 1234: the default route (2 n DLT hypotheses) and HAF proposals (members, stride) ==", flush=True)
    env = dict(os.environ, MULTIH_TIMING="1")
    r = subprocess.run(["timeout", "-k", "10", str(LIMITS["haf"] - 20), sys.executable, os.path.abspath(__file__), "haf_child"], env=env,
                       capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stdout[-3000:] + r.stderr[-3000:], flush=True)
        sys.exit(r.returncode)
    cur, stages, inside, hyp = None, [], False, 0
    for line in r.stdout.splitlines():
        if line.startswith("@@ end"):
            inside = False
        elif line.startswith("@@ result"):
            f = line.split()
            t = dict(stages)
            names = [s for s, _ in stages]
            before = stages[names.index("initial models") - 1][1] if "initial models" in names and names.index("initial models") > 0 else float("nan")
            init = t.get("initial models", float("nan")) - before
            table = t["HAF neighbour table"] - stages[names.index("HAF neighbour table") - 1][1] if "HAF neighbour table" in names else 0.0
            points, planes, source, members, stride = cur
            what = "default (DLT)  " if source == 0 else f"HAF ({members:2d}, {stride})    "
            print(f"{points:6d} / {planes:2d} {what}: hypotheses {hyp:6d}, clusters {f[3]:>2s}, planes {f[5]}/{planes}, ARI {f[7]}, loop iterations {f[9]}, "
                  f"neighbour table {table:.2f} ms, initial models {init:.2f} ms, Process() second call {f[11]} ms / median of five more {f[13]} ms", flush=True)
        elif line.startswith("@@ "):
            cur, stages, inside = tuple(int(v) for v in line.split()[1:]), [], True
            hyp = 2 * cur[0]                                      # the default route's; the HAF route's log line names its own
        elif inside:
            m = re.match(r"\[Multi-H\] (.+) done ([0-9.]+) ms after Process\(\) began", line)
            if m:
                stages.append((m.group(1), float(m.group(2))))
            m = re.match(r"\[Multi-H\] HAF proposals: (\d+) hypotheses", line)
            if m:
                hyp = int(m.group(1))


def barrsmith():
    B = importlib.import_module("barrsmith_agreement")
    host = _host()
    pts, ref_rows, ref_labels = B.kept_correspondences(with_rows=True)
    print("== raw barrsmith file, harness route (load filter 2 px, point-to-line distance), twelve seeds ==", flush=True)
    res = {}
    for source, members, name in ((0, 0, "default (DLT)"), (1, 16, "HAF (16, 1)"), (1, 32, "HAF (32, 1)")):
        res[name] = []
        for seed in SEEDS12:
            host.mhh_set_proposal_source(source, members, 1)
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
    elif part == "haf_child":
        haf_child()
    elif part in LIMITS:
        {"kernel": kernel, "default": lambda: default(parent), "haf": haf, "barrsmith": barrsmith}[part]()
    else:
        for part in LIMITS:
            cmd = ["timeout", "-k", "10", str(LIMITS[part]), sys.executable, os.path.abspath(__file__), part] + (["--parent", parent] if parent else [])
            r = subprocess.run(cmd)
            if r.returncode != 0:
                print(f"{part}: exit status {r.returncode}; the parts after it were not run", flush=True)
                sys.exit(r.returncode)
