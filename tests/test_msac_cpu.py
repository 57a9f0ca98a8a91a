"""CPU tests of the MSAC-weighted score: the numpy twin (tests/msac_numpy.py) against the oracle's counts and against known
answers, and what the libraries must export for it.  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import msac_numpy as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.eye(3).reshape(1, 9)
S_ZERO = np.array([1, 0, 0, 0, 1, 0, -0.5, 0, 1.0])            # s = 0 at the point (2, 1): d2 = inf
ZERO_OVER_ZERO = np.array([1, 0, -2.0, 0, 1, 0, -0.5, 0, 1.0])  # ... and 0 / 0: d2 = NaN


def test_twin_counts_are_the_oracles(synth, oracle):
    sc = synth.make_scene(4099, 3, seed=5, with_neighbours=False)
    rng = np.random.default_rng(5)
    H = list(sc.H_true)
    while len(H) < 65:
        if len(H) % 2:
            H.append(sc.H_true[len(H) % 3] * (1.0 + rng.normal(0, 1e-3, size=9)))
        else:
            H.append((np.eye(3) + rng.normal(0, 0.05, size=(3, 3))).reshape(9))
    H = np.ascontiguousarray(np.array(H))
    thr2 = 2.2 * 2.2
    mask = (rng.random(sc.n) < 0.7).astype(np.uint8)
    mask[:5] = 0
    mask[1020:1030] = 0
    for mk in (None, mask):
        cnt, wgt = W.score_msac(sc.src, sc.dst, H, thr2, mk)
        assert np.array_equal(cnt, oracle.score(sc.src, sc.dst, H, thr2, mk))
        assert cnt.max() > 500 and np.all(wgt <= W.SCALE * cnt) and np.all(wgt >= 0)
        assert np.all((wgt > 0) <= (cnt > 0))
    assert not np.array_equal(W.score_msac(sc.src, sc.dst, H, thr2)[0], W.score_msac(sc.src, sc.dst, H, thr2, mask)[0])


def _one(dst, thr2, H=IDENTITY, src=(0.0, 0.0)):
    cnt, wgt = W.score_msac(np.array([src]), np.array([dst]), H, thr2)
    return int(cnt[0]), int(wgt[0])


def test_known_answers_against_the_identity():
    assert _one((0.0, 0.0), 4.84) == (1, 256)                                   # d2 = 0
    assert _one((3.0, 0.0), np.nextafter(9.0, np.inf)) == (1, 0)                # d2 = nextafter(thr2, 0): counted, weighs 0
    assert _one((3.0, 0.0), 9.0) == (0, 0)                                      # d2 = thr2: not counted
    assert _one((3.0, 0.0), np.nextafter(9.0, 0.0)) == (0, 0)
    assert _one((5.0, 7.0), 1e300, H=S_ZERO.reshape(1, 9), src=(2.0, 1.0)) == (0, 0)          # inf
    assert _one((5.0, 7.0), 1e300, H=ZERO_OVER_ZERO.reshape(1, 9), src=(2.0, 1.0)) == (0, 0)  # NaN
    # halves away from zero: d2 / thr2 = 507 / 512 exactly, 256 (1 - q) = 2.5 -> 3 (half-to-even would give 2)
    assert 507.0 * 507.0 / 259584.0 == 507.0 / 512.0 and 256.0 * (1.0 - 507.0 / 512.0) == 2.5
    assert _one((507.0, 0.0), 259584.0) == (1, 3)
    # the same rule on bare d2 values
    thr2 = 4.84
    d2 = np.array([[0.0, np.nextafter(thr2, 0.0), thr2, np.inf, np.nan, thr2 / 2]])
    inl, w = W.pair_terms(d2, thr2)
    assert inl.tolist() == [[True, True, False, False, False, True]] and w.tolist() == [[256, 0, 0, 0, 0, 128]]
    assert W.best_by_weight([3, 7, 7, 1]) == 1


def test_null_engine_is_refused(engine_lib):
    """(the two symbols are what the parent library lacks)"""
    assert engine_lib.mh_score_msac(None, C.c_double(1.0), None, None, None) == -2
    assert engine_lib.mh_select_best_msac(None, None, None, None) == -2
    assert engine_lib.mh_get_model(None, 0, None) == -2


def test_header_constants_and_host_hook(mh, engine_lib):
    text = open(os.path.join(ROOT, "include", "multih_hip.h")).read()
    assert re.search(r"^#define\s+MH_MSAC_SCALE\s+256\s*$", text, flags=re.M)
    assert re.search(r"\bMH_BUF_WEIGHTS\s*=\s*7\b", text)
    assert mh.capi.MSAC_SCALE == W.SCALE == 256 and mh.capi.BUF_WEIGHTS == 7
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    assert hasattr(host, "mhh_set_tail_score")


def test_product_library_carries_the_msac_kernels(mh, engine_lib):
    raw = subprocess.run(["strings", mh.LIB_PATH], capture_output=True, text=True).stdout
    names = sorted({l for l in raw.splitlines() if re.match(r"^_ZN2mh\d+k_msac", l)})
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    kernels = sorted({re.sub(r"\(.*", "", d).replace("void ", "") for d in dem})
    assert [k for k in kernels if k.startswith("mh::k_msac32")] == ["mh::k_msac32<4, 64, false>", "mh::k_msac32<4, 64, true>"], kernels
    assert [k for k in kernels if k.startswith("mh::k_msac64")] == ["mh::k_msac64<false>", "mh::k_msac64<true>"], kernels
