#!/usr/bin/env python3
"""Are the kernels of two builds the same instructions?  Compiles HIP sources device-only to gfx950 assembly with the build's
flags and compares the BODY of every kernel (label to .Lfunc_end) after numbering away what depends on a kernel's place in its
file: the function index inside local labels (.LBB12_3 -> .LBB_3) and the compilation-unit hash.  No GPU.

    python tools/asm_kernel_diff.py --old old/expand.hip --new multi-h_amd/csrc/expand.hip multi-h_amd/csrc/expand_solve.hip

Prints one line per kernel; exit status 1 when a body differs or a kernel exists on one side only.  --detail adds, for a
kernel that differs, what differs: descriptor lines, mnemonic counts and a diff with register and block numbers masked."""
import argparse
import collections
import difflib
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


def detail(old, new):
    """What differs between two kernels that are not the same text: descriptor lines, the multiset of mnemonics, and the
    body as a unified diff with register and block numbers masked (v12, s[4:5], .LBB_7 -> v#, s#, .LBB_#), so that a
    renumbering alone shows nothing."""
    desc = lambda k: [l for l in k if l.startswith(".amdhsa_")]
    ops = lambda k: collections.Counter(l.split()[0] for l in k if not l.startswith(".") and not l.endswith(":"))
    for o, n in zip(desc(old), desc(new)):
        if o != n:
            print(f"    descriptor: {o}  ->  {n}")
    if desc(old) == desc(new):
        print("    descriptor: equal")
    a, b = ops(old), ops(new)
    diff = {m: (a[m], b[m]) for m in sorted(set(a) | set(b)) if a[m] != b[m]}
    print("    mnemonics: " + (", ".join(f"{m} {x} -> {y}" for m, (x, y) in diff.items()) if diff else "equal multiset"))
    raw = [l for l in difflib.unified_diff(old, new, n=0, lineterm="") if l[0] in "+-" and l[:3] not in ("+++", "---")]
    print(f"    text: {sum(l[0] == '-' for l in raw)} lines removed, {sum(l[0] == '+' for l in raw)} added; with register numbers masked:")
    regs = lambda k: [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])|(\.LBB_)\d+", r"\1\3#", l) for l in k if not l.startswith(".amdhsa_")]
    for l in difflib.unified_diff(regs(old), regs(new), "old", "new", n=0, lineterm=""):
        print("      " + l)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--include", default=b.CSRC, help="where the old sources find the headers they include")
    ap.add_argument("--detail", action="store_true", help="for a kernel that differs: descriptor, mnemonic counts, unified diff")
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
            if a.detail and not same:
                detail(old[name], new[name])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
