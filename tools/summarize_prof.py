#!/usr/bin/env python3
"""Condenses rocprofv3 CSV outputs (kernel stats + PMC passes) into a short text summary."""
import csv, glob, os, sys, collections
import hashlib, json
out = sys.argv[1]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = int(os.environ.get("WARMUP", "3")), int(os.environ.get("STEPS", "20"))
print("== source: HEAD", os.environ.get("HEAD_SHA", "unknown"), " bench_py_sha16", hashlib.sha256(open(os.path.join(ROOT, "bench.py"), "rb").read()).hexdigest()[:16],
      " libmultih_hip_sha16", hashlib.sha256(open(os.path.join(ROOT, "multi-h_amd", "libmultih_hip.so"), "rb").read()).hexdigest()[:16])
KEEP = [k for k in os.environ.get("KERNELS", "k_residual,k_dlt4").split(",") if k]
ROWS = int(os.environ.get("STAT_ROWS", "14"))
def materialising(name):
    """the product's materialising residual sweep, demangled or mangled: the kernel over the configuration mh::cfg::Sweep, on
    the resident grid or hardware-dispatched; in archived traces (r01-r05) the kernel with WRITE_R = true as its third
    template argument, at 16 or 64 models per work item"""
    return any(k in name for k in ("k_residual<mh::cfg::Sweep>", "k_residual_resident<mh::cfg::Sweep>",
                                   "k_residualINS_3cfg5SweepEEE", "k_residual_residentINS_3cfg5SweepEEE",
                                   "k_residual<4, 16, true", "k_residualILi4ELi16ELb1", "k_residual_resident<4, 16, true",
                                   "k_residual_residentILi4ELi16ELb1", "k_residual<4, 64, true", "k_residualILi4ELi64ELb1",
                                   "k_residual_resident<4, 64, true", "k_residual_residentILi4ELi64ELb1"))
def find(sub, pat):
    return sorted(glob.glob(os.path.join(out, sub, "**", pat), recursive=True))
for f in find("trace", "*kernel_stats.csv"):
    print("== kernel stats:", os.path.relpath(f, out))
    with open(f) as fh:
        for i, row in enumerate(csv.reader(fh)):
            if i < ROWS: print("  ", ",".join(row))
# Per-dispatch durations of the residual kernel from the kernel trace, in launch order: bench.py runs WARMUP untimed steps,
# then STEPS timed ones in the PIPELINED form (a DLT beside every sweep), then the same again in the SEQUENTIAL form.  r05: at one
# GPU the sequential form is the headline (bench.py `form`), so the average over ITS timed launches is what bench.py's own event
# timing reports as kernel_ms.k_residual and prices roofline.achieved with; the pipelined form's launches are printed beside it
# (`pipelined_form.k_residual_ms` of the bench line); warm-up launches are left out.
for f in find("trace", "*kernel_trace.csv"):
    durs = []
    with open(f) as fh:
        rows = [r for r in csv.DictReader(fh) if materialising(r.get("Kernel_Name", ""))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows]
    if len(durs) >= 2 * (WARMUP + STEPS):
        pipe = durs[WARMUP:WARMUP + STEPS]
        head = durs[2 * WARMUP + STEPS: 2 * WARMUP + 2 * STEPS]
        N, M = 50000, 100000
        alg = 8.0 * N * M + 32.0 * N + 72.0 * M + 4.0 * M
        print(f"== k_residual (materialising) dispatches in the trace: {len(durs)}; HEADLINE timed region (sequential form) = launches "
              f"{2 * WARMUP + STEPS + 1}..{2 * WARMUP + 2 * STEPS}: avg {sum(head) / len(head):.4f} ms, min {min(head):.4f}, max {max(head):.4f}")
        print(f"   -> {alg / (sum(head) / len(head) * 1e-3) / 1e9:.1f} GB/s = {alg / (sum(head) / len(head) * 1e-3) / 8e12:.4f} of the 8 TB/s peak (algorithmic {alg / 1e9:.4f} GB per launch)")
        print(f"   pipelined form (a DLT beside every sweep), launches {WARMUP + 1}..{WARMUP + STEPS}: avg {sum(pipe) / len(pipe):.4f} ms = "
              f"{alg / (sum(pipe) / len(pipe) * 1e-3) / 8e12:.4f} of the peak; the run's first {WARMUP} (warm-up) launches: {', '.join(f'{d:.3f}' for d in durs[:WARMUP])} ms")
traffic = {}
for sub in ("pmc_fetch", "pmc_write", "pmc_sq", "pmc_sq2", "pmc_label"):
    for f in find(sub, "*counter_collection.csv"):
        agg = collections.defaultdict(lambda: [0, 0.0])
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "?")
                name = name[:name.index("(")] if "(" in name else name      # keep the template arguments: variants differ there
                k = (name.replace("void ", "")[:100], row.get("Counter_Name", "?"))
                agg[k][0] += 1
                agg[k][1] += float(row.get("Counter_Value", 0) or 0)
        print("== PMC:", os.path.relpath(f, out))
        for (kn, cn), (n, tot) in sorted(agg.items()):
            if any(k in kn for k in KEEP):
                print(f"   {kn:92s} {cn:24s} launches={n:4d} avg={tot/n:.6g}")
            if materialising(kn) and cn in ("FETCH_SIZE", "WRITE_SIZE"):
                traffic[cn] = (tot / n, n)
if "FETCH_SIZE" in traffic and "WRITE_SIZE" in traffic:
    w = traffic["WRITE_SIZE"][0] * 1024.0
    fcorr = traffic["FETCH_SIZE"][0] * 1024.0 * 2.0
    rec = {"points": 50000, "models": 100000, "kernel": "k_residual", "hbm_bytes_per_launch": w + fcorr, "write_bytes": w,
           "fetch_bytes_corrected": fcorr, "launches_averaged": traffic["WRITE_SIZE"][1], "head": os.environ.get("HEAD_SHA", "unknown"),
           "method": "rocprofv3 --pmc WRITE_SIZE and --pmc FETCH_SIZE in separate passes (tools/profile_bench.sh); KiB -> bytes; FETCH_SIZE doubled per MI355X_MICROARCH.md (gfx950 counts 128-B requests at 64 B)"}
    with open(os.path.join(out, "residual_traffic.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print("== HBM traffic of k_residual per launch:", json.dumps(rec))
