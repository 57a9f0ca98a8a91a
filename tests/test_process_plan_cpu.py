"""MultiH::PlanRun without a GPU and without an engine: the checks of Process() that depend only on the settings and on which
optional entry points the engine library has, called directly by tests/process_plan_caller.cpp (compiled with the host sources and
the stand-in engine, which is never created here).  One wrong setting per case and the message Process() has always written for
it; every optional mode against a library that lacks its entry points; pairs of wrong settings, for the order of the checks; and
the values of the plan."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

import label_cost_numpy as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "multi-h_amd", "host")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_plan_run_checks_and_plans_as_process_always_did(tmp_path):
    srcs = [os.path.join(ROOT, "tests", "process_plan_caller.cpp"), os.path.join(ROOT, "tests", "fake_engine.cpp"),
            *importlib.import_module("multi-h_amd.build").HOST_SOURCES]
    exe = str(tmp_path / "caller")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-ffp-contract=off", "-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                        *srcs, "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "FAILED" not in r.stdout
    m = re.search(r"process_plan_caller ok: (\d+) checks", r.stdout)
    assert m and int(m.group(1)) >= 100, r.stdout[-500:]
    assert r.stderr == "", "PlanRun prints nothing"
    # SetLabelCost in energy units: llround(points * round(lam * T)) at lambda 0.5, thr_hom 2.2 (tests/test_label_cost_cpu.py: 4901 per outlier)
    beta = {float(p): int(v) for p, v in re.findall(r"^beta (\S+) (-?\d+)$", r.stdout, re.M)}
    assert beta == {40.0: L.beta_of(40.0, 0.5, 2.2 ** 2), 0.5: L.beta_of(0.5, 0.5, 2.2 ** 2)}
    assert beta == {40.0: 196040, 0.5: 2451}
