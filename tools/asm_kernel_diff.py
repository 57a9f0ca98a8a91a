#!/usr/bin/env python3
"""Are the kernels of two builds the same instructions?  Compiles HIP sources device-only to gfx950 assembly with the build's
flags and compares the BODY of every kernel (label to .Lfunc_end) after numbering away what depends on a kernel's place in its
file: the function index inside local labels (.LBB12_3 -> .LBB_3) and the compilation-unit hash.  No GPU.

    python tools/asm_kernel_diff.py --old old/expand.hip --new multi-h_amd/csrc/expand.hip multi-h_amd/csrc/expand_solve.hip

Prints one line per kernel; exit status 1 when a body differs or a kernel exists on one side only."""
import argparse
import hashlib
import importlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
b = importlib.import_module("multi-h_amd.build")


def kernels(src, include, tmp):
    out = os.path.join(tmp, hashlib.sha1(os.path.abspath(src).encode()).hexdigest()[:10] + ".s")
    subprocess.run([b.HIPCC] + b.HIP_FLAGS + ["--offload-device-only", "-S", "-I" + include, src, "-o", out], check=True)
    text = open(out).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    found = {}
    for name in names:
        m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, flags=re.M | re.S)
        body = [re.sub(r"\s*;.*", "", l).rstrip() for l in m.group(0).splitlines()[1:-1]]
        body = [re.sub(r"\.L(BB|tmp|func_begin|func_end)\d+", r".L\1", l) for l in body if l.strip()]
        body = [re.sub(r"__hip_cuid_\w+", "__hip_cuid", l) for l in body]
        # ... and the kernel descriptor behind it (registers, LDS, scratch)
        d = re.search(r"^\s*\.amdhsa_kernel\s+%s\n(.*?)^\s*\.end_amdhsa_kernel" % re.escape(name), text, flags=re.M | re.S)
        found[name] = body + [l.strip() for l in d.group(1).splitlines()]
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--include", default=b.CSRC, help="where the old sources find the headers they include")
    a = ap.parse_args()
    old, new = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for s in a.old:
            old.update(kernels(s, a.include, tmp))
        for s in a.new:
            new.update(kernels(s, b.CSRC, tmp))
    dem = subprocess.run(["c++filt"], input="\n".join(sorted(set(old) | set(new))), capture_output=True, text=True).stdout.splitlines()
    bad = 0
    for name, pretty in zip(sorted(set(old) | set(new)), dem):
        pretty = re.sub(r"\(.*", "", pretty).replace("void ", "")
        if name not in old or name not in new:
            print(f"{pretty:48s} only in the {'new' if name in new else 'old'} build")
            bad += 1
        else:
            same = old[name] == new[name]
            bad += not same
            print(f"{pretty:48s} {len(old[name]):6d} / {len(new[name]):6d} lines  {'identical' if same else 'DIFFERENT'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
