"""The 3-point proposer's twin (tests/propose_3pt_numpy.py) against the oracle, what a 3-point batch is worth to the selection
beside the DLT batch from the same tuples, and what the built libraries must offer.  No GPU: the engine's batches are compared
with this twin in tests/test_gpu_propose_3pt.py."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import propose_3pt_numpy as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "multi-h_amd", "host")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_library_exports_the_entry_point(mh, engine_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", mh.LIB_PATH], capture_output=True, text=True).stdout
    assert "mh_propose_3pt" in set(re.findall(r" T (mh_\w+)", out))
    assert "mh_propose_3pt" in mh.SYMBOLS
    header = open(os.path.join(ROOT, "include", "multih_hip.h")).read()
    assert re.search(r"MH_API int mh_propose_3pt\(mh_engine\* e, unsigned long long seed, long long first, int m\);", header)
    assert "#define MH_ABI_VERSION 2" in header
    # the host class refers to it weakly: an engine library without it still loads
    host = os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so")
    out = subprocess.run(["nm", "-D", host], capture_output=True, text=True).stdout
    assert re.search(r"\bw mh_propose_3pt\b", out), "mh_propose_3pt must be a weak reference of libmultih_host.so"
    assert "PROPOSAL_SOURCE_3PT = 2" in open(os.path.join(HOST, "MultiH.h")).read()


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_the_host_class_accepts_source_2_and_says_so_without_the_entry_point(tmp_path):
    """MultiH over tests/fake_engine.cpp, an engine without mh_propose_3pt: it links (the reference is weak), source 2 is a
    known source that fails with its own message — with affinities and point-only —, source 7 is unknown, and the default route
    gives the same clusters before and after."""
    srcs = [os.path.join(ROOT, "tests", "propose_3pt_caller.cpp"), os.path.join(ROOT, "tests", "fake_engine.cpp"),
            *importlib.import_module("multi-h_amd.build").HOST_SOURCES]
    exe = str(tmp_path / "caller")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-ffp-contract=off", "-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                        *srcs, "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, MULTIH_ENGINE_POOL="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "propose_3pt_caller ok" in r.stdout
    assert r.stderr.count("the engine library has no 3-point proposals (mh_propose_3pt)") == 2
    assert "unknown proposal source 7 (PROPOSAL_SOURCE_DLT or PROPOSAL_SOURCE_HAF)" in r.stderr


def test_the_harness_takes_3pt_without_arguments(mh, engine_lib, tmp_path):
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    assert os.path.exists(harness), "harness not built"
    for bad in ("3pt:4", "3pt:x", "3pt:", "3pts"):
        r = subprocess.run([harness, str(tmp_path / "in.txt"), str(tmp_path / "out.txt"), "--proposals", bad],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
        assert f"--proposals {bad}: dlt, 3pt, haf, haf:members or haf:members:stride" in r.stderr, r.stderr
    r = subprocess.run([harness], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--proposals dlt|haf[:members[:stride]]|3pt]" in r.stderr
    # the value itself is taken: the run gets as far as the input file, which is not there (no GPU is touched before that)
    for extra in ([], ["--points"]):
        r = subprocess.run([harness, str(tmp_path / "missing.txt"), str(tmp_path / "out.txt"), "--proposals", "3pt", *extra],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--proposals" not in r.stderr and "missing.txt" in r.stderr, (r.returncode, r.stderr)


def test_the_kernel_uses_no_scratch(mh, tmp_path):
    """k_propose_3pt takes its uniform tuple from the shared sample_tuple<3, 64>, whose indexed out[got++] stays in registers only
    because the compiler promotes the three-element array.  Held here: csrc/propose3pt.hip compiled device-only with the build's
    flags must report, for BOTH instantiations, scratch 0, no spilled register, no dynamic stack and no LDS."""
    import importlib
    b = importlib.import_module("multi-h_amd.build")
    r = subprocess.run([b.HIPCC] + b.HIP_FLAGS + ["--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                  os.path.join(b.CSRC, "propose3pt.hip"), "-o", str(tmp_path / "propose3pt.s")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    kernels = {}
    for blk in blocks:
        name = blk.split()[0]
        kernels[name] = {k.strip(): v.strip() for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+): (\S+) \[-Rpass", blk)}
    mine = {n: f for n, f in kernels.items() if "k_propose_3pt" in n}
    print({n: (f.get("VGPRs"), f.get("TotalSGPRs"), f.get("Occupancy [waves/SIMD]")) for n, f in mine.items()})
    assert len(mine) == 2, sorted(kernels)
    for name, f in mine.items():
        assert f["ScratchSize [bytes/lane]"] == "0" and f["VGPRs Spill"] == "0" and f["SGPRs Spill"] == "0", (name, f)
        assert f["Dynamic Stack"] == "False" and f["LDS Size [bytes/block]"] == "0", (name, f)


def test_tuples_are_the_first_three_of_the_samplers(mh, oracle):
    import local_sampler_numpy as L
    sc = mh.synth.make_scene(64, 3, seed=5, with_neighbours=False)
    nbr = L.knn_table(sc.src, sc.dst, 8)
    assert np.array_equal(twin.tuples(7, 3, 200, sc.n), oracle.sample4(7, 3, 200, sc.n)[:, :3])
    for u in (0, 4):
        assert np.array_equal(twin.tuples(7, 3, 200, sc.n, nbr, u), L.sample_local(7, 3, 200, sc.n, nbr, u)[:, :3])
    assert np.array_equal(twin.tuples(7, 3, 200, sc.n, nbr, 16), twin.tuples(7, 3, 200, sc.n))
    # the first three of a 4-tuple are sample_tuple<3, 64>: the same draws, the same rejections, n = 3 included (one possible set)
    three = twin.tuples(11, 0, 50, 3)
    assert (np.sort(three, axis=1) == np.array([0, 1, 2])).all()
    want = np.array([L.uniform_tuple(11, c, 3)[:3] for c in range(50)])
    assert np.array_equal(three, want)
    s4 = twin.samples(three)
    assert s4.shape == (50, 4) and s4.dtype == np.int32 and (s4[:, 3] == -1).all() and np.array_equal(s4[:, :3], three)
    assert twin.tuples(1, 0, 0, 10).shape == (0, 3)


def test_fits_equal_the_oracles_unrefined_3pt(mh, engine_lib, oracle):
    """The twin's fit (the host library's Homography3PTLinear) against oracle.homography_3pt(refine=False) on 1 000 uniform
    tuples of make_scene(600, 3, seed=99) under the scene's true F: measured BIT-EQUAL, 1 000 of 1 000 rows, every fit
    succeeding on both sides — so the assertion is equality, not a tolerance."""
    host = twin.host_lib(mh.LIB_PATH)
    sc = mh.synth.make_scene(600, 3, seed=99, with_neighbours=False)
    idx3 = twin.tuples(1234, 0, 1000, sc.n)
    H, ok = twin.fit(host, sc.src, sc.dst, sc.F, idx3)
    ref = [oracle.homography_3pt(sc.src[t], sc.dst[t], sc.F, refine=False) for t in idx3]
    H_ref, ok_ref = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
    same = (_bits(H) == _bits(H_ref)).all(axis=1)
    print(f"fits succeeding: twin {int(ok.sum())}, oracle {int(ok_ref.sum())} of 1000; rows bit-equal: {int(same[ok].sum())}")
    assert np.array_equal(ok, ok_ref) and ok.sum() >= 990
    assert same[ok].all()
    # a failed fit is nine quiet NaNs: three times the same correspondence has no homography
    Hd, okd = twin.fit(host, sc.src, sc.dst, sc.F, np.array([[5, 5, 5]], dtype=np.int32))
    assert not okd[0] and (_bits(Hd) == 0x7ff8000000000000).all()


# ---- what the selection makes of the two batches (the nine cells of the issue's second table) ------------------------------
THR2, NEED, MAX_MODELS, TUPLE_SEED = 2.5 ** 2, 20, 16, 5


def _covered(oracle, sc, Hs):
    """Planes of which one selected model holds at least half of the points within the threshold."""
    if len(Hs) == 0:
        return set()
    with np.errstate(all="ignore"):
        d2 = oracle.residual_matrix(sc.src, sc.dst, Hs)
    out = set()
    for p in range(int(sc.gt_label.max()) + 1):
        own = sc.gt_label == p
        if ((d2[:, own] < THR2).sum(axis=1) >= 0.5 * own.sum()).any():
            out.add(p)
    return out


@pytest.mark.parametrize("n,planes,seed", [(2000, 5, 99), (5000, 10, 99), (3000, 3, 36)])
def test_the_selection_covers_no_fewer_planes_than_from_the_dlt_batch(mh, engine_lib, oracle, n, planes, seed):
    """oracle.select_greedy (thr 2.5, need 20, at most 16 models, no refit) over the DLT batch and over the 3-point batch built
    from the SAME tuples (oracle.sample4, seed 5; the 3-point batch takes their first three indices and the scene's true F), at
    M = 2n, n/2 and n/5.  Measured, planes covered DLT / 3-point:
        2 000 / 5, seed 99    {2,3} / {0,1,2,3}    {2,3} / {2,3}    {2,3} / {2,3}
        5 000 / 10, seed 99   6 / 9                2 / 8            0 / 4
        3 000 / 3, seed 36    3 / 3                3 / 3            2 / 3"""
    host = twin.host_lib(mh.LIB_PATH)
    sc = mh.synth.make_scene(n, planes, seed=seed, with_neighbours=False)
    for M in (2 * n, n // 2, n // 5):
        idx = oracle.sample4(TUPLE_SEED, 0, M, n)
        H_dlt = oracle.dlt4(sc.src, sc.dst, idx)[0]
        H_3pt, ok = twin.fit(host, sc.src, sc.dst, sc.F, np.ascontiguousarray(idx[:, :3]))
        with np.errstate(all="ignore"):
            sel_dlt = oracle.select_greedy(sc.src, sc.dst, H_dlt, THR2, NEED, MAX_MODELS)
            sel_3pt = oracle.select_greedy(sc.src, sc.dst, H_3pt, THR2, NEED, MAX_MODELS)
        c_dlt, c_3pt = _covered(oracle, sc, sel_dlt[0]), _covered(oracle, sc, sel_3pt[0])
        print(f"{n} / {planes}, seed {seed}, M = {M}: DLT {sorted(c_dlt)} ({len(sel_dlt[0])} models), "
              f"3-point {sorted(c_3pt)} ({len(sel_3pt[0])} models), {int((~ok).sum())} fits failed")
        assert len(c_3pt) >= len(c_dlt), (n, planes, seed, M)
