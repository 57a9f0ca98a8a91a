"""The symmetric route (mh_set_residual_scope, MultiH::SetResidual) without a GPU: that the scenes the GPU tests use tell the
two errors apart, what the built libraries must offer, and the host class over an engine library without the entry points.
The engine's outputs are compared with the twin (tests/symmetric_route_numpy.py) in tests/test_gpu_symmetric_route.py."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import data_term_numpy as T
import symmetric_route_numpy as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "multi-h_amd", "host")
LAM = 0.5
SCENES = [(300, 3, 2, 1.0), (2000, 5, 3, 1.0), (2000, 5, 3, 0.5)]          # n, planes, seed, thr_hom


def scene_models(sc, seed):
    return sc.H_true * (1.0 + np.random.default_rng(seed).normal(0, 1e-4, size=sc.H_true.shape))


@pytest.mark.parametrize("n,k,seed,thr", SCENES)
def test_the_scenes_tell_the_two_errors_apart(mh, oracle, n, k, seed, thr):
    """Cold labeling (lambda 0.5, the scene's own hit graph) under the forward and under the symmetric table, and the points
    inside thr^2 by one error and not by the other.  Measured, energy forward / symmetric, sites whose label differs, such
    points per model: 300/3 at 1.0: 208 750 / 205 643, 2, 13-25; 2000/5 at 1.0: 969 171 / 963 794, 1, 31-150; 2000/5 at 0.5:
    503 154 / 506 000, 229, 24-88 (the current scene generator, mh.synth, not the parity suite's).  Asserted: the inequalities."""
    sc = mh.synth.make_scene(n, k, seed=seed)
    H = scene_models(sc, seed)
    thr2 = thr * thr
    lab = np.full(sc.n, -1, dtype=np.int32)
    fwd = T.labeling_step_twin(sc.src, sc.dst, sc.aff, H, LAM, thr2, sc.hit_rowptr, sc.hit_col, False, sc.F, sc.e2, lab, T.REFERENCE)
    sym = S.labeling_step_twin(sc.src, sc.dst, sc.aff, H, LAM, thr2, sc.hit_rowptr, sc.hit_col, False, sc.F, sc.e2, lab, S.REFERENCE)
    with np.errstate(all="ignore"):
        d2f, d2s = oracle.residual_matrix(sc.src, sc.dst, H), S.sym_d2(sc.src, sc.dst, H)
    only_fwd = ((d2f < thr2) & ~(d2s < thr2)).sum(axis=1)
    differing = int((fwd[0] != sym[0]).sum())
    table_share = float((T.cost_table(sc.src, sc.dst, H, LAM, thr2, T.REFERENCE) != S.cost_table(sc.src, sc.dst, H, LAM, thr2)).mean())
    print(f"{n}/{k} seed {seed} thr {thr}: energy {fwd[2]} / {sym[2]}, {differing} sites differ, forward-only inliers per model "
          f"{int(only_fwd.min())}-{int(only_fwd.max())}, {100 * table_share:.1f} % of the table differs")
    assert fwd[2] != sym[2]
    assert differing >= 1
    assert only_fwd.min() >= 10
    assert not ((d2s < thr2) & ~(d2f < thr2)).any(), "a symmetric inlier is a forward inlier"


def test_the_twin_is_the_header_table_on_the_symmetric_error(mh, oracle):
    sc = mh.synth.make_scene(300, 3, seed=2)
    H = scene_models(sc, 2)
    d2 = S.sym_d2(sc.src, sc.dst, H)
    d2f = oracle.residual_matrix(sc.src, sc.dst, H)
    # forward + backward, one rounded addition: the backward term is the forward error of adj(H) on the swapped pair
    adj = np.array([[h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
                     h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
                     h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]] for h in H])
    back = np.array([oracle.residual_matrix(sc.dst, sc.src, adj[m:m + 1])[0] for m in range(len(H))])
    assert np.array_equal((d2f + back).view(np.uint64), d2.view(np.uint64))
    for term in (S.REFERENCE, S.RISING):
        table = S.cost_table(sc.src, sc.dst, H, LAM, 1.0, term)
        assert table.dtype == np.int32 and table.shape == (sc.n, len(H) + 1)
        assert (table[:, 0] == T.outlier_cost(LAM, 1.0)).all()
        assert np.array_equal(table[:, 1:].T, T.term_of_d2(d2, LAM, 1.0, term))
        assert np.array_equal(S.cost_matrix(sc.src, sc.dst, H, LAM, 1.0, term), table[:, 1:].T)


def test_the_library_exports_the_entry_point(mh, engine_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", mh.LIB_PATH], capture_output=True, text=True).stdout
    assert "mh_set_residual_scope" in set(re.findall(r" T (mh_\w+)", out))
    assert "mh_set_residual_scope" in mh.SYMBOLS and hasattr(mh.Engine, "set_residual_scope")
    header = open(os.path.join(ROOT, "include", "multih_hip.h")).read()
    assert re.search(r"MH_API int mh_set_residual_scope\(mh_engine\* e, int scope\);", header)
    assert "#define MH_RESIDUAL_SCOPE_SCORE 0" in header and "#define MH_RESIDUAL_SCOPE_ROUTE 1" in header
    assert "#define MH_ABI_VERSION 2" in header
    assert "always use the forward formula" not in header
    # a null engine is refused before anything touches a device
    assert engine_lib.mh_set_residual_scope(None, 0) == -2 and engine_lib.mh_set_residual_scope(None, 1) == -2
    # the host class refers to both setters weakly: an engine library without them still loads
    host = os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so")
    out = subprocess.run(["nm", "-D", host], capture_output=True, text=True).stdout
    assert re.search(r"\bw mh_set_residual_scope\b", out) and re.search(r"\bw mh_set_residual_mode\b", out)
    assert re.search(r" T mhh_set_residual\b", out)
    assert "RESIDUAL_FORWARD = 0, RESIDUAL_SYMMETRIC = 1" in open(os.path.join(HOST, "MultiH.h")).read()


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_the_host_class_over_an_engine_without_the_entry_points(tmp_path):
    """MultiH over tests/fake_engine.cpp, an engine without mh_set_residual_mode / mh_set_residual_scope: it links (the
    references are weak), the forward route runs as before, RESIDUAL_SYMMETRIC fails with its message, an unknown value and
    the MSAC tail together with the symmetric error are refused, and the default route gives the same clusters afterwards."""
    srcs = [os.path.join(ROOT, "tests", "symmetric_route_caller.cpp"), os.path.join(ROOT, "tests", "fake_engine.cpp"),
            *importlib.import_module("multi-h_amd.build").HOST_SOURCES]
    exe = str(tmp_path / "caller")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-ffp-contract=off", "-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                        *srcs, "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, MULTIH_ENGINE_POOL="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "symmetric_route_caller ok" in r.stdout
    assert r.stderr.count("the engine library has no symmetric route (mh_set_residual_mode, mh_set_residual_scope)") == 1
    assert "unknown residual 7 (RESIDUAL_FORWARD or RESIDUAL_SYMMETRIC)" in r.stderr
    assert "they do not combine with RESIDUAL_SYMMETRIC" in r.stderr


def test_the_harness_takes_the_residual_flag(mh, engine_lib, tmp_path):
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    assert os.path.exists(harness), "harness not built"
    r = subprocess.run([harness, str(tmp_path / "in.txt"), str(tmp_path / "out.txt"), "--residual", "bogus"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "--residual: forward or symmetric" in r.stderr
    r = subprocess.run([harness], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--residual forward|symmetric]" in r.stderr
    # the value itself is taken: the run gets as far as the input file, which is not there (no GPU is touched before that)
    for word in ("forward", "symmetric"):
        r = subprocess.run([harness, str(tmp_path / "missing.txt"), str(tmp_path / "out.txt"), "--residual", word],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--residual" not in r.stderr and "missing.txt" in r.stderr, (r.returncode, r.stderr)


def test_the_new_kernels_use_no_scratch(mh, tmp_path):
    """The symmetric instantiations of the four kernels behind the selection, compiled device-only with the build's flags:
    no scratch, no spilled register, no dynamic stack."""
    import importlib
    b = importlib.import_module("multi-h_amd.build")
    want = {"k_data_cost": 2, "k_cost_matrix": 2, "k_moments": 1, "k_inliers_of_model": 1}
    seen = {k: 0 for k in want}
    for unit in ("datacost.hip", "residual.hip"):
        r = subprocess.run([b.HIPCC] + b.HIP_FLAGS + ["--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                      os.path.join(b.CSRC, unit), "-o", str(tmp_path / (unit + ".s"))],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        names = re.findall(r"remark: Function Name: (\S+)", r.stderr)
        pretty = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
        for blk, name in zip(re.split(r"remark: Function Name: ", r.stderr)[1:], pretty):
            m = re.match(r"void mh::(k_data_cost|k_cost_matrix|k_moments|k_inliers_of_model)<(.*?)>\(", name)
            if not m or not m.group(2).endswith("true"):       # SYM is the last template argument
                continue
            f = {k.strip(): v.strip() for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+): (\S+) \[-Rpass", blk)}
            print(name.split("(")[0], f.get("VGPRs"), f.get("TotalSGPRs"), f.get("LDS Size [bytes/block]"), f.get("Occupancy [waves/SIMD]"))
            assert f["ScratchSize [bytes/lane]"] == "0" and f["VGPRs Spill"] == "0" and f["SGPRs Spill"] == "0", (name, f)
            assert f["Dynamic Stack"] == "False", (name, f)
            seen[m.group(1)] += 1
    assert seen == want
