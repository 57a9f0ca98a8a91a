"""The selectable data term without a GPU: the entry point exists in header, binding and library; the numpy twin
(tests/data_term_numpy.py) is the oracle under MH_DATA_TERM_REFERENCE — table, LabelingStep and the whole merge <-> label
loop — and has the properties the header states under MH_DATA_TERM_RISING."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import data_term_numpy as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR, LOCALITY = 2.2, 0.005
THR2 = THR * THR


def test_entry_point_is_declared_bound_and_exported(mh, engine_lib):
    header = open(os.path.join(ROOT, "include", "multih_hip.h")).read()
    assert re.search(r"MH_API\s+int\s+mh_set_data_term\s*\(\s*mh_engine\s*\*\s*e\s*,\s*int\s+term\s*\)\s*;", header)
    assert re.search(r"#define\s+MH_DATA_TERM_REFERENCE\s+0\b", header) and re.search(r"#define\s+MH_DATA_TERM_RISING\s+1\b", header)
    assert re.search(r"#define\s+MH_ABI_VERSION\s+2\b", header), "purely additive: the ABI version stays 2"
    assert "mh_set_data_term" in mh.SYMBOLS and hasattr(mh.Engine, "set_data_term")
    assert hasattr(engine_lib, "mh_set_data_term")
    assert engine_lib.mh_set_data_term(None, 1) == -2          # MH_ERR_INVALID: a null engine, before anything touches a device
    assert engine_lib.mh_set_data_term(None, 0) == -2
    assert engine_lib.mh_abi_version() == 2


@pytest.fixture(scope="module")
def scene(synth):
    sc = synth.make_scene(300, 3, seed=2)
    rng = np.random.default_rng(2)
    H = [sc.H_true * (1.0 + rng.normal(0, 1e-4, size=sc.H_true.shape))]
    for _ in range(2):                                         # near-copies: the mean shift merges them -> a `changed` iteration
        k = rng.integers(0, 3)
        H.append(sc.H_true[k:k + 1] * (1.0 + rng.normal(0, 2e-4, size=(1, 9))))
    H.append((np.eye(3) + rng.normal(0, 0.05, size=(3, 3))).reshape(1, 9))      # a stray nothing supports
    return sc, np.ascontiguousarray(np.concatenate(H, axis=0))


@pytest.mark.parametrize("lam", [0.5, 0.3])
def test_reference_table_is_the_oracles(scene, oracle, lam):
    sc, H0 = scene
    H = np.concatenate([H0, np.eye(3).reshape(1, 9), np.array([[1, 0, 0, 0, 1, 0, -0.5, 0, 1.0]])])
    src = sc.src.copy()
    src[0] = (2.0, 0.0)                                        # s = 0 for the last model: a non-finite d2
    want = oracle.data_cost(src, sc.dst, H, lam, THR2)
    got = T.cost_table(src, sc.dst, H, lam, THR2, T.REFERENCE)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert want[0, -1] == 2 * T.outlier_cost(lam, THR2)


def test_reference_labeling_step_is_the_oracles(scene, oracle):
    sc, H0 = scene
    lab_t = lab_o = np.full(sc.n, -1, np.int32)
    H_t = H_o = H0[:3]
    for it in range(3):
        warm = it > 0
        lab_o, H_o, e_o, c_o = oracle.labeling_step(sc.src, sc.dst, sc.aff, H_o, 0.5, THR2, sc.hit_rowptr, sc.hit_col, warm, sc.F, sc.e2, lab_o)
        lab_t, H_t, e_t, c_t = T.labeling_step_twin(sc.src, sc.dst, sc.aff, H_t, 0.5, THR2, sc.hit_rowptr, sc.hit_col, warm, sc.F,
                                                    sc.e2, lab_t, T.REFERENCE)
        assert (e_t, c_t) == (e_o, c_o) and np.array_equal(lab_t, lab_o), it
        assert np.array_equal(H_t.view(np.uint64), H_o.view(np.uint64)), it


@pytest.mark.parametrize("use_reference_gco", [False, True])
def test_reference_loop_is_the_oracles(scene, oracle, use_reference_gco):
    sc, H0 = scene
    lab_o, H_o, it_o, en_o, _ = oracle.cluster_merging_and_labeling(sc.src, sc.dst, sc.aff, H0, sc.F, sc.e2, 0.5, THR, sc.hit_rowptr,
                                                                    sc.hit_col, 2, use_reference_gco=use_reference_gco)
    lab_t, H_t, it_t, en_t = T.loop_twin(sc.src, sc.dst, sc.aff, H0, sc.F, sc.e2, 0.5, THR, sc.hit_rowptr, sc.hit_col, 2, T.REFERENCE)
    assert it_o >= 2 and H_o.shape[0] >= 2 and en_o > 0, "the scene should run the loop, not leave by an early exit"
    assert (it_t, en_t) == (it_o, en_o) and np.array_equal(lab_t, lab_o)
    assert H_t.shape == H_o.shape and np.array_equal(H_t.view(np.uint64), H_o.view(np.uint64))


def test_loop_twin_early_exits_are_the_oracles(scene, oracle):
    """One cluster (:280-285) and none: no LabelingStep runs, so the data term cannot show."""
    sc, H0 = scene
    for H in (H0[:1], np.zeros((0, 9))):
        lab_o, H_o, it_o, en_o, _ = oracle.cluster_merging_and_labeling(sc.src, sc.dst, sc.aff, H, sc.F, sc.e2, 0.5, THR, sc.hit_rowptr,
                                                                        sc.hit_col, 3)
        for term in (T.REFERENCE, T.RISING):
            lab_t, H_t, it_t, en_t = T.loop_twin(sc.src, sc.dst, sc.aff, H, sc.F, sc.e2, 0.5, THR, sc.hit_rowptr, sc.hit_col, 3, term)
            assert (it_t, en_t) == (it_o, en_o) and np.array_equal(lab_t, lab_o) and np.array_equal(H_t, H_o)


@pytest.mark.parametrize("lam", [0.5, 0.3])
def test_rising_term_properties(lam):
    lam_ = 100.0 / lam
    Tt = THR2 * 81.0 / 16.0
    B = T.outlier_cost(lam, THR2)
    below = np.nextafter(Tt, 0.0)
    rise = lambda d2: T.term_of_d2(d2, lam, THR2, T.RISING)
    ref = lambda d2: T.term_of_d2(d2, lam, THR2, T.REFERENCE)
    assert rise(0.0) == 0 and ref(0.0) == int(T.c_round(lam_))
    assert rise(below) == int(T.c_round(lam_)), "the largest double below T"
    for d2 in (Tt, np.nextafter(Tt, np.inf), 1e300, np.inf, np.nan):
        assert rise(d2) == 2 * B and ref(d2) == 2 * B, d2
    rng = np.random.default_rng(0)
    d2 = np.sort(np.concatenate([rng.uniform(0, Tt, 200000), Tt * (1.0 - 2.0 ** -np.arange(1, 53)), Tt * 2.0 ** -np.arange(1, 200.0),
                                 Tt * (np.arange(0, 2 * int(lam_) + 2) / (2.0 * lam_)), [0.0, below]]))
    d2 = d2[d2 < Tt]
    r, f = rise(d2).astype(np.int64), ref(d2).astype(np.int64)
    assert np.all(np.diff(r) >= 0), "non-decreasing in d2"
    assert np.all(np.diff(f) <= 0)
    assert r.min() == 0 and r.max() == int(T.c_round(lam_)) < B
    # two roundings of complementary values
    assert set(np.unique(r + f).tolist()) <= {int(T.c_round(lam_)) - 1, int(T.c_round(lam_)), int(T.c_round(lam_)) + 1}


def test_c_round_is_half_away_from_zero():
    x = np.array([0.0, 0.49999999999999994, 0.5, 1.5, 2.5, 3.5, 199.5, 200.5, 2.4999999999999996])
    assert T.c_round(x).tolist() == [0, 0, 1, 2, 3, 4, 200, 201, 2]
    assert np.round(2.5) == 2.0, "np.round rounds halves to even: the reason it is not used"


def test_expansion_of_a_rising_table_reference_gco_and_oracle_agree(scene, oracle):
    if oracle.ref() is None:
        pytest.skip("oracle/_ref is not built")
    sc, H0 = scene
    for lam in (0.5, 0.3):
        cost = T.cost_table(sc.src, sc.dst, H0, lam, THR2, T.RISING)
        assert not np.array_equal(cost, T.cost_table(sc.src, sc.dst, H0, lam, THR2, T.REFERENCE))
        lab, energy, cycles, _ = oracle.expand(cost, sc.hit_rowptr, sc.hit_col, oracle.potts(lam))
        lab_r, e_r = oracle.ref_expand_table(cost, sc.hit_rowptr, sc.hit_col, oracle.potts(lam))
        assert energy == e_r and np.array_equal(lab, lab_r)
        assert len(np.unique(lab)) >= 3
