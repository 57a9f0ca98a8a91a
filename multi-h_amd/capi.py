"""ctypes binding of include/multih_hip.h (libmultih_hip.so) for tests, bench
and multi-GPU plumbing.  One method per C entry point, numpy in / numpy out; no
computation happens in Python and nothing here falls back to the CPU: if the
library is missing or no gfx950 device is visible, construction raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MH_LIB: another build of the same ABI, e.g. the measurement library of `build.py --tuning` (tools/ only)
LIB_PATH = os.environ.get("MH_LIB") or os.path.join(HERE, "libmultih_hip.so")

MH_OK = 0
ERR_NAMES = {-1: "MH_ERR_NO_DEVICE", -2: "MH_ERR_INVALID", -3: "MH_ERR_HIP", -4: "MH_ERR_NOT_SET",
             -5: "MH_ERR_OVERFLOW"}
BUF_COUNTS, BUF_MODELS, BUF_RESIDUALS, BUF_LABELS, BUF_COST, BUF_LABEL_COUNTS, BUF_WEIGHTS = 0, 1, 2, 3, 4, 6, 7
MSAC_SCALE = 256                       # MH_MSAC_SCALE
ESTIMATORS = {"haf": 0, "3pt": 1, "dlt": 2}      # MH_ESTIMATOR_HAF, MH_ESTIMATOR_3PT, MH_ESTIMATOR_DLT
SAMPLER_UNIFORM, SAMPLER_LOCAL = 0, 1  # MH_SAMPLER_UNIFORM, MH_SAMPLER_LOCAL
RESIDUAL_SCOPES = {"score": 0, "route": 1}      # MH_RESIDUAL_SCOPE_SCORE, MH_RESIDUAL_SCOPE_ROUTE
DATA_TERMS = {"reference": 0, "rising": 1}      # MH_DATA_TERM_REFERENCE, MH_DATA_TERM_RISING
SMOOTH_RULES = {"uniform": 0, "cauchy": 1}      # MH_SMOOTH_UNIFORM, MH_SMOOTH_CAUCHY
MERGE_OK, MERGE_EMPTY, MERGE_NO_FIT = 0, 1, 2   # MH_MERGE_*
MERGE_NO_DELTA = 2**63 - 1                      # LLONG_MAX: the delta of a pair that is not OK
DROP_OK, DROP_EMPTY = 0, 1                      # MH_DROP_*
DROP_NO_DELTA = 2**63 - 1                       # LLONG_MAX: the delta of a candidate that is not OK
BEST_ALT_TILE = 64                              # models per LDS tile of k_best_alternative (csrc/mh_kernels.hpp)
K_DLT4, K_RESIDUAL, K_SCORE, K_DATACOST, K_EXPAND, K_REESTIMATE, K_COSTMATRIX = 0, 1, 2, 3, 4, 5, 6

# every symbol include/multih_hip.h declares (tests check the export table against this)
SYMBOLS = [
    "mh_abi_version", "mh_last_error", "mh_device_count", "mh_create", "mh_destroy", "mh_set_params",
    "mh_set_stream", "mh_synchronize", "mh_set_correspondences", "mh_set_epipolar",
    "mh_set_neighbors_csr", "mh_build_neighbors_knn", "mh_build_neighbors_knn_radius", "mh_build_neighbors_radius", "mh_get_sym_graph", "mh_get_sym_multiplicity", "mh_set_smoothness_weights", "mh_set_fundamental_metric", "mh_propose_fund8",
    "mh_get_fund_hypotheses", "mh_score_sampson", "mh_refit_fundamental", "mh_estimate_fundamental", "mh_propose_fund7", "mh_get_fund7_samples", "mh_estimate_fundamental_minimal", "mh_epipoles", "mh_refine_correspondences", "mh_get_refine_reasons", "mh_refine_points",
    "mh_local_homographies", "mh_mean_shift", "mh_propose_dlt4",
    "mh_set_models", "mh_get_models", "mh_get_model_count", "mh_get_model", "mh_get_samples", "mh_set_sampler", "mh_build_sample_neighbours", "mh_get_sample_neighbours", "mh_propose_haf", "mh_get_haf_support", "mh_propose_3pt", "mh_set_residual_mode", "mh_set_residual_scope", "mh_score", "mh_score_msac", "mh_select_best_msac",
    "mh_residual_matrix", "mh_cost_matrix", "mh_get_residual_rows", "mh_set_transport", "mh_select_greedy", "mh_select_greedy_msac", "mh_get_score_stats", "mh_prefetch_dlt4", "mh_adopt_prefetched", "mh_select_best", "mh_get_copy_stats", "mh_inliers_of_model", "mh_inliers_of_homography", "mh_refit_homography", "mh_polish_homographies", "mh_reweight_homographies", "mh_label_residual_quantile", "mh_reweight_homographies_auto", "mh_compat_trial_stats", "mh_compat_trial_stats_fit", "mh_compat_dlt_medians", "mh_inlier_moments", "mh_set_data_term", "mh_data_cost", "mh_expand",
    "mh_get_expand_stats", "mh_get_expand_batch_stats", "mh_get_expand_trace", "mh_get_core_components", "mh_set_estimator", "mh_set_estimator_reweighting", "mh_set_estimator_reweighting_auto", "mh_reestimate", "mh_labeling_step", "mh_merge_deltas", "mh_labeling_energy", "mh_best_alternative", "mh_drop_deltas", "mh_device_buffer", "mh_profile_enable", "mh_profile_reset",
    "mh_profile_get", "mh_set_tuning",
]


class MultiHError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


_lib = None


def load_library(path: str | None = None) -> C.CDLL:
    """dlopen the engine; raises (never falls back) when it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise FileNotFoundError(f"{p} is not built; run `python multi-h_amd/build.py` "
                                "(or __graft_entry__.build())")
    lib = C.CDLL(p)
    lib.mh_last_error.restype = C.c_char_p
    lib.mh_destroy.restype = None
    if path is None:
        _lib = lib
    return lib


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Engine:
    """Thin owner of one `mh_engine*`."""

    def __init__(self, device: int = 0, thr_fund_mat: float = 3.0, thr_hom: float = 2.5,
                 locality: float = 0.002, lam: float = 0.5, min_inliers: int = 0):
        self.lib = load_library()
        self._h = C.c_void_p()
        self._check(self.lib.mh_create(C.byref(self._h), int(device)))
        self.n = 0
        self.set_params(thr_fund_mat, thr_hom, locality, lam, min_inliers)

    # -- plumbing -----------------------------------------------------------
    def _check(self, rc: int) -> None:
        if rc != MH_OK:
            raise MultiHError(rc, (self.lib.mh_last_error() or b"").decode())

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.mh_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- parameters / inputs ------------------------------------------------
    def set_params(self, thr_fund_mat, thr_hom, locality, lam, min_inliers=0):
        self._check(self.lib.mh_set_params(self._h, C.c_double(thr_fund_mat), C.c_double(thr_hom),
                                           C.c_double(locality), C.c_double(lam), int(min_inliers)))
        self.thr_hom, self.lam = float(thr_hom), float(lam)

    def set_stream(self, stream_ptr: int | None, external: bool = True):
        """Launch on the caller's hipStream_t (0 / None = the HIP default stream); external=False
        returns to the engine's own stream."""
        self._check(self.lib.mh_set_stream(self._h, C.c_void_p(stream_ptr or 0), int(bool(external))))

    def synchronize(self):
        self._check(self.lib.mh_synchronize(self._h))

    def set_correspondences(self, src, dst, aff=None):
        src, dst = _f64(src), _f64(dst)
        n = src.shape[0]
        ap = None
        if aff is not None:
            aff = _f64(aff).reshape(n, 4)
            ap = _p(aff, C.c_double)
        self._check(self.lib.mh_set_correspondences(self._h, _p(src, C.c_double), _p(dst, C.c_double), ap, n))
        self.n = n

    def set_epipolar(self, F, e2):
        F, e2 = _f64(F).reshape(9), _f64(e2).reshape(2)
        self._check(self.lib.mh_set_epipolar(self._h, _p(F, C.c_double), _p(e2, C.c_double)))

    def set_neighbors_csr(self, rowptr, col):
        rowptr, col = _i32(rowptr), _i32(col)
        cp = _p(col, C.c_int) if col.size else None
        self._check(self.lib.mh_set_neighbors_csr(self._h, _p(rowptr, C.c_int), cp, rowptr.size - 1))

    def build_neighbors_knn(self, k: int, radius: float = 0.0):
        """k nearest hits per query; radius > 0 keeps only those within it (the reference's 1/locality)."""
        if radius > 0.0:
            self._check(self.lib.mh_build_neighbors_knn_radius(self._h, int(k), C.c_double(radius)))
        else:
            self._check(self.lib.mh_build_neighbors_knn(self._h, int(k)))

    def build_neighbors_radius(self, radius: float, max_hits: int = 0) -> int:
        hits = C.c_longlong(0)
        self._check(self.lib.mh_build_neighbors_radius(self._h, C.c_double(radius), C.c_longlong(max_hits), C.byref(hits)))
        return int(hits.value)

    def get_sym_graph(self):
        nnz = C.c_int(0)
        self._check(self.lib.mh_get_sym_graph(self._h, None, None, None, C.byref(nnz)))
        rp = np.empty(self.n + 1, dtype=np.int32)
        col = np.empty(nnz.value, dtype=np.int32)
        w = np.empty(nnz.value, dtype=np.int32)
        self._check(self.lib.mh_get_sym_graph(self._h, _p(rp, C.c_int), _p(col, C.c_int), _p(w, C.c_int), None))
        return rp, col, w

    def sym_multiplicity(self):
        """mh_get_sym_multiplicity: the hit multiplicities of get_sym_graph()'s arcs, whatever smoothness rule is in force."""
        nnz = C.c_int(0)
        self._check(self.lib.mh_get_sym_graph(self._h, None, None, None, C.byref(nnz)))
        mult = np.empty(nnz.value, dtype=np.int32)
        self._check(self.lib.mh_get_sym_multiplicity(self._h, _p(mult, C.c_int)))
        return mult

    def set_smoothness_weights(self, rule, rho: float = 0.0, q_max: int = 1):
        """mh_set_smoothness_weights: "uniform" (default; w = multiplicity) or "cauchy" (w = multiplicity x
        max(1, round(q_max rho^2 / (rho^2 + d))), d the float32 squared distance of the arc's sites); sticky, applies to the
        resident graph at once and to every later one."""
        if isinstance(rule, str):
            if rule not in SMOOTH_RULES:
                raise ValueError(f"unknown smoothness rule {rule!r}")
            rule = SMOOTH_RULES[rule]
        self._check(self.lib.mh_set_smoothness_weights(self._h, int(rule), C.c_double(rho), int(q_max)))

    # -- epipolar front half ---------------------------------------------------
    def propose_fund8(self, seed: int, first: int, m: int):
        self._check(self.lib.mh_propose_fund8(self._h, C.c_ulonglong(seed), C.c_longlong(first), int(m)))
        self._fm = int(m)

    def get_fund_hypotheses(self):
        F = np.empty((self._fm, 9), dtype=np.float64)
        idx = np.empty((self._fm, 8), dtype=np.int32)
        self._check(self.lib.mh_get_fund_hypotheses(self._h, _p(F, C.c_double), _p(idx, C.c_int)))
        return F, idx

    def propose_fund7(self, seed: int, first: int, m: int):
        """m minimal 7-point samples, up to three F each: the hypothesis set then has 3 m slots (NaN where there is no solution)."""
        self._check(self.lib.mh_propose_fund7(self._h, C.c_ulonglong(seed), C.c_longlong(first), int(m)))
        self._fm = 3 * int(m)
        self._f7m = int(m)

    def get_fund7_hypotheses(self):
        """The 3 m slots of the last propose_fund7 as an (m, 3, 9) array."""
        F = np.empty((self._fm, 9), dtype=np.float64)
        self._check(self.lib.mh_get_fund_hypotheses(self._h, _p(F, C.c_double), None))
        return F.reshape(-1, 3, 9)

    def get_fund7_samples(self):
        idx = np.empty((self._f7m, 7), dtype=np.int32)
        nvalid = np.empty(self._f7m, dtype=np.int32)
        self._check(self.lib.mh_get_fund7_samples(self._h, _p(idx, C.c_int), _p(nvalid, C.c_int)))
        return idx, nvalid

    def score_sampson(self, thr2: float):
        cnt = np.empty(self._fm, dtype=np.int32)
        self._check(self.lib.mh_score_sampson(self._h, C.c_double(thr2), _p(cnt, C.c_int)))
        return cnt

    def refit_fundamental(self, F, thr2: float, iterations: int = 1):
        F = _f64(F).reshape(9)
        out = np.empty(9, dtype=np.float64)
        mask = np.empty(self.n, dtype=np.uint8)
        inl = C.c_int(0)
        self._check(self.lib.mh_refit_fundamental(self._h, _p(F, C.c_double), C.c_double(thr2), int(iterations),
                                                  _p(out, C.c_double), _p(mask, C.c_ubyte), C.byref(inl)))
        return out, mask, inl.value

    def set_fundamental_metric(self, metric: int) -> None:
        """0 = Sampson (default), 1 = the larger squared point-to-epipolar-line distance (cv::findFundamentalMat's)."""
        self._check(self.lib.mh_set_fundamental_metric(self._h, int(metric)))

    def estimate_fundamental(self, seed: int, hypotheses: int, thr: float):
        F = np.empty(9, dtype=np.float64)
        e2 = np.empty(2, dtype=np.float64)
        mask = np.empty(self.n, dtype=np.uint8)
        inl = C.c_int(0)
        self._check(self.lib.mh_estimate_fundamental(self._h, C.c_ulonglong(seed), int(hypotheses), C.c_double(thr),
                                                     _p(F, C.c_double), _p(e2, C.c_double), _p(mask, C.c_ubyte),
                                                     C.byref(inl)))
        return F, e2, mask, inl.value

    def estimate_fundamental_minimal(self, seed: int, max_samples: int, confidence: float, thr: float):
        """7-point samples, confidence stop, no refit (cv::findFundamentalMat's scheme): F, e2, mask, inliers, samples_used."""
        F = np.empty(9, dtype=np.float64)
        e2 = np.empty(2, dtype=np.float64)
        mask = np.empty(self.n, dtype=np.uint8)
        inl, used = C.c_int(0), C.c_int(0)
        self._fm, self._f7m = 3 * int(max_samples), int(max_samples)      # (the proposal stands even where the estimate fails)
        self._check(self.lib.mh_estimate_fundamental_minimal(self._h, C.c_ulonglong(seed), int(max_samples), C.c_double(confidence),
                                                             C.c_double(thr), _p(F, C.c_double), _p(e2, C.c_double),
                                                             _p(mask, C.c_ubyte), C.byref(inl), C.byref(used)))
        return F, e2, mask, inl.value, used.value

    def epipoles(self, F):
        F = _f64(F).reshape(9)
        e1, e2 = np.empty(2), np.empty(2)
        self._check(self.lib.mh_epipoles(self._h, _p(F, C.c_double), _p(e1, C.c_double), _p(e2, C.c_double)))
        return e1, e2

    def refine_correspondences(self, F, e1, e2, in_mask=None):
        F, e1, e2 = _f64(F).reshape(9), _f64(e1).reshape(2), _f64(e2).reshape(2)
        keep = np.empty(self.n, dtype=np.uint8)
        out = np.empty((self.n, 8), dtype=np.float64)
        mp = None
        if in_mask is not None:
            in_mask = np.ascontiguousarray(in_mask, dtype=np.uint8)
            mp = _p(in_mask, C.c_ubyte)
        self._check(self.lib.mh_refine_correspondences(self._h, _p(F, C.c_double), _p(e1, C.c_double), _p(e2, C.c_double),
                                                       mp, _p(keep, C.c_ubyte), _p(out, C.c_double)))
        return keep, out

    def refine_points(self, F, e1, e2, in_mask=None):
        """mh_refine_points: the Hartley-Sturm correction alone, no affinities.  Returns (keep [n], refined [n, 4])."""
        F, e1, e2 = _f64(F).reshape(9), _f64(e1).reshape(2), _f64(e2).reshape(2)
        keep = np.empty(self.n, dtype=np.uint8)
        out = np.empty((self.n, 4), dtype=np.float64)
        mp = None
        if in_mask is not None:
            in_mask = np.ascontiguousarray(in_mask, dtype=np.uint8)
            mp = _p(in_mask, C.c_ubyte)
        self._check(self.lib.mh_refine_points(self._h, _p(F, C.c_double), _p(e1, C.c_double), _p(e2, C.c_double),
                                              mp, _p(keep, C.c_ubyte), _p(out, C.c_double)))
        return keep, out

    def refine_reasons(self):
        """Per row of the last refine_correspondences / refine_points call: 0 kept, 1 not in the mask, 2 triangulation,
        3 affine test."""
        r = np.empty(self.n, dtype=np.uint8)
        self._check(self.lib.mh_get_refine_reasons(self._h, _p(r, C.c_ubyte), int(self.n)))
        return r

    # -- reference-style initialisation ------------------------------------------
    def local_homographies(self, locality: float):
        H = np.empty((self.n, 9), dtype=np.float64)
        feat = np.empty((self.n, 10), dtype=np.float64)
        self._check(self.lib.mh_local_homographies(self._h, C.c_double(locality), _p(H, C.c_double), _p(feat, C.c_double)))
        return H, feat

    def mean_shift(self, data, band_width: float, seed: int):
        data = _f64(data)
        n, d = data.shape
        modes = np.empty((n, d), dtype=np.float64)
        assign = np.empty(n, dtype=np.int32)
        k = C.c_int(0)
        self._check(self.lib.mh_mean_shift(self._h, _p(data, C.c_double), n, d, C.c_double(band_width),
                                           C.c_ulonglong(seed), _p(modes, C.c_double), n, _p(assign, C.c_int), C.byref(k)))
        return modes[:k.value].copy(), assign, k.value

    # -- propose ------------------------------------------------------------
    def propose_dlt4(self, seed: int, first: int, m: int):
        self._check(self.lib.mh_propose_dlt4(self._h, C.c_ulonglong(seed), C.c_longlong(first), int(m)))

    def set_models(self, H):
        H = _f64(H).reshape(-1, 9)
        self._check(self.lib.mh_set_models(self._h, _p(H, C.c_double), H.shape[0]))

    @property
    def model_count(self) -> int:
        m = C.c_int(0)
        self._check(self.lib.mh_get_model_count(self._h, C.byref(m)))
        return m.value

    def get_models(self):
        H = np.empty((self.model_count, 9), dtype=np.float64)
        self._check(self.lib.mh_get_models(self._h, _p(H, C.c_double)))
        return H

    def get_model(self, idx: int):
        """mh_get_model: one model of the current set."""
        H = np.empty(9, dtype=np.float64)
        self._check(self.lib.mh_get_model(self._h, int(idx), _p(H, C.c_double)))
        return H

    def get_samples(self):
        idx = np.empty((self.model_count, 4), dtype=np.int32)
        self._check(self.lib.mh_get_samples(self._h, _p(idx, C.c_int)))
        return idx

    def set_sampler(self, sampler: int, uniform_per_16: int = 0):
        """mh_set_sampler: SAMPLER_UNIFORM (default) or SAMPLER_LOCAL (needs build_sample_neighbours); sticky."""
        self._check(self.lib.mh_set_sampler(self._h, int(sampler), int(uniform_per_16)))

    def build_sample_neighbours(self, k: int):
        """mh_build_sample_neighbours: the local sampler's n x k table (the labeling graph is not touched)."""
        self._check(self.lib.mh_build_sample_neighbours(self._h, int(k)))

    def get_sample_neighbours(self):
        k = C.c_int(0)
        self._check(self.lib.mh_get_sample_neighbours(self._h, None, C.byref(k)))
        nbr = np.empty((self.n, k.value), dtype=np.int32)
        self._check(self.lib.mh_get_sample_neighbours(self._h, _p(nbr, C.c_int), None))
        return nbr

    def propose_haf(self, first: int, m: int, stride: int = 1, members: int = 0, thr2: float = 0.0):
        """mh_propose_haf: m hypotheses, one per affine correspondence (anchors (first + s) * stride), refitted to the consistent
        ones among the first `members` neighbours of the sampling table (members = 0: the single correspondence)."""
        self._check(self.lib.mh_propose_haf(self._h, C.c_longlong(int(first)), int(m), int(stride), int(members), C.c_double(thr2)))

    def propose_3pt(self, seed: int, first: int, m: int):
        """mh_propose_3pt: m F-constrained 3-point hypotheses, counters first .. first + m - 1; the tuple of a counter is the
        first three indices of the 4-tuple the sampler (set_sampler) gives it.  Needs set_epipolar."""
        self._check(self.lib.mh_propose_3pt(self._h, C.c_ulonglong(seed), C.c_longlong(first), int(m)))

    def get_haf_support(self):
        """mh_get_haf_support: per hypothesis of the resident HAF batch the bit mask of its consistent neighbours (uint32)."""
        used = np.zeros(self.model_count, dtype=np.uint32)
        self._check(self.lib.mh_get_haf_support(self._h, _p(used, C.c_uint)))
        return used

    # -- score --------------------------------------------------------------
    def set_residual_mode(self, symmetric: bool):
        self._check(self.lib.mh_set_residual_mode(self._h, 1 if symmetric else 0))

    def set_residual_scope(self, name: str):
        """mh_set_residual_scope: "score" (default: the score family follows set_residual_mode) or "route" (so do data_cost,
        labeling_step, cost_matrix, inlier_moments and inliers_of_model / _of_homography); sticky, marks the data cost stale."""
        if name not in RESIDUAL_SCOPES:
            raise ValueError(f"unknown residual scope {name!r}; one of {sorted(RESIDUAL_SCOPES)}")
        self._check(self.lib.mh_set_residual_scope(self._h, RESIDUAL_SCOPES[name]))

    def score(self, thr2: float, mask=None, fetch: bool = True):
        cnt = np.empty(self.model_count, dtype=np.int32) if fetch else None
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            mp = _p(mask, C.c_ubyte)
        self._check(self.lib.mh_score(self._h, C.c_double(thr2), mp, _p(cnt, C.c_int) if fetch else None))
        return cnt

    def score_msac(self, thr2: float, mask=None, fetch: bool = True):
        """mh_score_msac: (counts, weights) per model — mh_score's counts and the MSAC weights; fetch=False leaves both on the device."""
        m = self.model_count
        cnt = np.empty(m, dtype=np.int32) if fetch else None
        wgt = np.empty(m, dtype=np.int32) if fetch else None
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            mp = _p(mask, C.c_ubyte)
        self._check(self.lib.mh_score_msac(self._h, C.c_double(thr2), mp, _p(cnt, C.c_int) if fetch else None,
                                           _p(wgt, C.c_int) if fetch else None))
        return cnt, wgt

    def select_best_msac(self):
        """mh_select_best_msac: (index, weight, count) of the model with the highest weight, the lowest index on ties."""
        idx, wgt, cnt = C.c_longlong(0), C.c_int(0), C.c_int(0)
        self._check(self.lib.mh_select_best_msac(self._h, C.byref(idx), C.byref(wgt), C.byref(cnt)))
        return int(idx.value), int(wgt.value), int(cnt.value)

    def residual_matrix(self, thr2: float, fetch_R: bool = True, fetch_counts: bool = True):
        m = self.model_count
        R = np.empty((m, self.n), dtype=np.float64) if fetch_R else None
        cnt = np.empty(m, dtype=np.int32) if fetch_counts else None
        self._check(self.lib.mh_residual_matrix(self._h, C.c_double(thr2),
                                                _p(R, C.c_double) if fetch_R else None,
                                                _p(cnt, C.c_int) if fetch_counts else None))
        return R, cnt

    def cost_matrix(self, fetch_C: bool = True, fetch_counts: bool = True):
        """mh_cost_matrix: int32 data cost of every model against every point (model-major), fused inlier counts."""
        m = self.model_count
        Cm = np.empty((m, self.n), dtype=np.int32) if fetch_C else None
        cnt = np.empty(m, dtype=np.int32) if fetch_counts else None
        self._check(self.lib.mh_cost_matrix(self._h, _p(Cm, C.c_int) if fetch_C else None, _p(cnt, C.c_int) if fetch_counts else None))
        return Cm, cnt

    def get_residual_rows(self, first: int, count: int):
        rows = np.empty((count, self.n), dtype=np.float64)
        self._check(self.lib.mh_get_residual_rows(self._h, int(first), int(count), _p(rows, C.c_double)))
        return rows

    def select_greedy(self, thr2: float, need: int, max_models: int, mask=None, total_m: int = 0):
        """Greedy selection over the resident batch on the device (mh_select_greedy, one rank).
        Returns (H [k,9], counters [k], counts [k], mask_out or None)."""
        H = np.zeros((int(max_models), 9))
        counters = np.zeros(int(max_models), dtype=np.int64)
        counts = np.zeros(int(max_models), dtype=np.int32)
        k = C.c_int(0)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).copy()
        self._check(self.lib.mh_select_greedy(self._h, C.c_double(thr2), int(need), int(max_models),
                                              None if m is None else m.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                              _p(H, C.c_double), counters.ctypes.data_as(C.POINTER(C.c_longlong)),
                                              _p(counts, C.c_int), C.byref(k), C.c_longlong(int(total_m))))
        return H[:k.value].copy(), counters[:k.value].copy(), counts[:k.value].copy(), m

    def select_greedy_msac(self, thr2: float, need: int, max_models: int, mask=None, total_m: int = 0):
        """The greedy selection ranked by MSAC weight (mh_select_greedy_msac): eligible with count >= need, the highest weight wins.
        Returns (H [k,9], counters [k], counts [k], weights [k], mask_out or None)."""
        H = np.zeros((int(max_models), 9))
        counters = np.zeros(int(max_models), dtype=np.int64)
        counts = np.zeros(int(max_models), dtype=np.int32)
        weights = np.zeros(int(max_models), dtype=np.int32)
        k = C.c_int(0)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).copy()
        self._check(self.lib.mh_select_greedy_msac(self._h, C.c_double(thr2), int(need), int(max_models),
                                                   None if m is None else m.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                   _p(H, C.c_double), counters.ctypes.data_as(C.POINTER(C.c_longlong)),
                                                   _p(counts, C.c_int), _p(weights, C.c_int), C.byref(k), C.c_longlong(int(total_m))))
        return H[:k.value].copy(), counters[:k.value].copy(), counts[:k.value].copy(), weights[:k.value].copy(), m

    def set_transport(self, rank: int, world: int, stream_fn=None, host_fn=None, ctx=None):
        """mh_set_transport: stream_fn = a C function pointer that enqueues the all-gather on the engine's stream
        (mhr_allgather of libmultih_rccl.so), host_fn = a host-synchronised ctypes hook (sharding.make_allgather_hook)."""
        self._transport_keepalive = (stream_fn, host_fn, ctx)
        self._check(self.lib.mh_set_transport(self._h, int(rank), int(world), C.cast(stream_fn, C.c_void_p) if stream_fn else None,
                                              C.cast(host_fn, C.c_void_p) if host_fn else None,
                                              ctx if isinstance(ctx, C.c_void_p) else C.c_void_p(ctx or 0)))

    def prefetch_dlt4(self, seed: int, first: int, m: int):
        self._check(self.lib.mh_prefetch_dlt4(self._h, C.c_ulonglong(seed), C.c_longlong(first), int(m)))

    def adopt_prefetched(self):
        self._check(self.lib.mh_adopt_prefetched(self._h))

    def select_best(self, total_m: int = 0, fetch: bool = True):
        """(index in the whole batch, count) of the best-supported model; fetch=False only enqueues."""
        if not fetch:
            self._check(self.lib.mh_select_best(self._h, C.c_longlong(int(total_m)), None, None))
            return None
        idx, cnt = C.c_longlong(0), C.c_int(0)
        self._check(self.lib.mh_select_best(self._h, C.c_longlong(int(total_m)), C.byref(idx), C.byref(cnt)))
        return int(idx.value), int(cnt.value)

    def score_stats(self, reset=False):
        """(pairs scored through the FP32 pre-test, pairs among them that needed the FP64 formula)"""
        a, b = C.c_longlong(0), C.c_longlong(0)
        self._check(self.lib.mh_get_score_stats(self._h, C.byref(a), C.byref(b), int(bool(reset))))
        return int(a.value), int(b.value)

    def copy_stats(self, reset=False):
        a, b = C.c_longlong(0), C.c_longlong(0)
        self._check(self.lib.mh_get_copy_stats(self._h, C.byref(a), C.byref(b), int(bool(reset))))
        return int(a.value), int(b.value)

    def inliers_of_model(self, idx: int, thr2: float, label_value: int, labels):
        labels = _i32(labels).copy()
        self._check(self.lib.mh_inliers_of_model(self._h, int(idx), C.c_double(thr2), int(label_value),
                                                 _p(labels, C.c_int)))
        return labels

    def inliers_of_homography(self, H, thr2: float, label_value: int, labels):
        labels = _i32(labels).copy()
        H = np.ascontiguousarray(H, dtype=np.float64).reshape(9)
        self._check(self.lib.mh_inliers_of_homography(self._h, _p(H, C.c_double), C.c_double(thr2), int(label_value),
                                                      _p(labels, C.c_int)))
        return labels

    def refit_homography(self, H, thr2: float, iterations: int):
        """mh_refit_homography: H refitted to all its inliers, at most `iterations` rounds in one launch; the model set is left
        untouched.  Returns (H_out [9], mask uint8 [n], inliers, fits_accepted)."""
        H = np.ascontiguousarray(H, dtype=np.float64).reshape(9)
        out = np.empty(9, dtype=np.float64)
        mask = np.empty(self.n, dtype=np.uint8)
        inl, acc = C.c_int(0), C.c_int(0)
        self._check(self.lib.mh_refit_homography(self._h, _p(H, C.c_double), C.c_double(thr2), int(iterations),
                                                 _p(out, C.c_double), _p(mask, C.c_ubyte), C.byref(inl), C.byref(acc)))
        return out, mask, inl.value, acc.value

    def polish_homographies(self, labels, H, max_iterations: int):
        """mh_polish_homographies: every row of H (m x 9) polished by Levenberg-Marquardt over the correspondences that carry its
        label, all iterations in one launch; the model set is left untouched.  Returns (H_out [m, 9], cost [m, 2] = S before and
        after, info int32 [m, 4] = members, iterations run, steps accepted, status)."""
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if labels.size != self.n:
            raise ValueError(f"labels: {labels.size} values for {self.n} correspondences")
        H = np.ascontiguousarray(H, dtype=np.float64).reshape(-1, 9)
        m = H.shape[0]
        out = np.empty((m, 9), dtype=np.float64)
        cost = np.empty((m, 2), dtype=np.float64)
        info = np.empty((m, 4), dtype=np.int32)
        self._check(self.lib.mh_polish_homographies(self._h, _p(labels, C.c_int), _p(H, C.c_double), m, int(max_iterations),
                                                    _p(out, C.c_double), _p(cost, C.c_double), _p(info, C.c_int)))
        return out, cost, info

    def reweight_homographies(self, labels, H, c2: float, rounds: int):
        """mh_reweight_homographies: every row of H (m x 9) refitted by `rounds` reweighted N-point DLT rounds over the
        correspondences that carry its label, weights 1 - d2 / c2, all rounds in one launch; the model set is left untouched.
        Returns (H_out [m, 9], gain [m, 2] = W under H_in and under H_out, info int32 [m, 4] = members, support of H_out,
        rounds done, status)."""
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if labels.size != self.n:
            raise ValueError(f"labels: {labels.size} values for {self.n} correspondences")
        H = np.ascontiguousarray(H, dtype=np.float64).reshape(-1, 9)
        m = H.shape[0]
        out = np.empty((m, 9), dtype=np.float64)
        gain = np.empty((m, 2), dtype=np.float64)
        info = np.empty((m, 4), dtype=np.int32)
        self._check(self.lib.mh_reweight_homographies(self._h, _p(labels, C.c_int), _p(H, C.c_double), m, C.c_double(c2), int(rounds),
                                                      _p(out, C.c_double), _p(gain, C.c_double), _p(info, C.c_int)))
        return out, gain, info

    def label_residual_quantile(self, labels, H, num: int, den: int):
        """mh_label_residual_quantile: per row of H (m x 9) the element at rank ((c - 1) * num) / den of the ascending forward
        transfer errors of the c correspondences that carry its label (1/2: the lower median).  Returns (d2 [m] — the quiet
        NaN for a label without members —, info int32 [m, 4] = members, rank, members strictly below the value, status)."""
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if labels.size != self.n:
            raise ValueError(f"labels: {labels.size} values for {self.n} correspondences")
        H = np.ascontiguousarray(H, dtype=np.float64).reshape(-1, 9)
        m = H.shape[0]
        d2 = np.empty(m, dtype=np.float64)
        info = np.empty((m, 4), dtype=np.int32)
        self._check(self.lib.mh_label_residual_quantile(self._h, _p(labels, C.c_int), _p(H, C.c_double), m, int(num), int(den),
                                                        _p(d2, C.c_double), _p(info, C.c_int)))
        return d2, info

    def reweight_homographies_auto(self, labels, H, num: int, den: int, kappa2: float, c2_min: float, c2_max: float, rounds: int):
        """mh_reweight_homographies_auto: reweight_homographies with c2 = clamp(kappa2 * the (num, den) order statistic of the
        label's errors under the model that stands, c2_min, c2_max), re-estimated in every round.  Returns (H_out [m, 9],
        gain [m, 2] = W under H_in and under H_out, each at its own scale, scale [m, 2] = c2 under H_in and under H_out,
        info int32 [m, 4] = members, support of H_out, rounds done, status)."""
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if labels.size != self.n:
            raise ValueError(f"labels: {labels.size} values for {self.n} correspondences")
        H = np.ascontiguousarray(H, dtype=np.float64).reshape(-1, 9)
        m = H.shape[0]
        out = np.empty((m, 9), dtype=np.float64)
        gain = np.empty((m, 2), dtype=np.float64)
        scale = np.empty((m, 2), dtype=np.float64)
        info = np.empty((m, 4), dtype=np.int32)
        self._check(self.lib.mh_reweight_homographies_auto(self._h, _p(labels, C.c_int), _p(H, C.c_double), m, int(num), int(den),
                                                           C.c_double(kappa2), C.c_double(c2_min), C.c_double(c2_max), int(rounds),
                                                           _p(out, C.c_double), _p(gain, C.c_double), _p(scale, C.c_double),
                                                           _p(info, C.c_int)))
        return out, gain, scale, info

    def inlier_moments(self, thr2: float):
        m = self.model_count
        mo = np.empty((m, 6), dtype=np.float64)
        me = np.empty(m, dtype=np.float64)
        self._check(self.lib.mh_inlier_moments(self._h, C.c_double(thr2), _p(mo, C.c_double), _p(me, C.c_double)))
        return mo, me

    # -- label --------------------------------------------------------------
    def data_cost(self, fetch: bool = True):
        cost = np.empty((self.n, self.model_count + 1), dtype=np.int32) if fetch else None
        self._check(self.lib.mh_data_cost(self._h, _p(cost, C.c_int) if fetch else None))
        return cost

    def expand(self, init_labels=None):
        labels = np.empty(self.n, dtype=np.int32)
        ip = None
        if init_labels is not None:
            init_labels = _i32(init_labels)
            ip = _p(init_labels, C.c_int)
        energy, cycles = C.c_int(0), C.c_int(0)
        self._check(self.lib.mh_expand(self._h, ip, _p(labels, C.c_int), C.byref(energy), C.byref(cycles)))
        return labels, energy.value, cycles.value

    def compat_trial_stats(self, pts_xyxy, cluster_begin, tri, H, ok):
        """mh_compat_trial_stats: per (cluster, trial) the five middle order statistics and the three largest squared
        transfer errors.  tri [clusters, trials, 3], H [clusters, trials, 9], ok [clusters, trials]."""
        pts = _f64(pts_xyxy).reshape(-1, 4)
        begin = np.ascontiguousarray(cluster_begin, dtype=np.int32)
        tri = np.ascontiguousarray(tri, dtype=np.int32)
        clusters, trials = tri.shape[0], tri.shape[1]
        H = _f64(H).reshape(clusters, trials, 9)
        ok = np.ascontiguousarray(ok, dtype=np.uint8).reshape(clusters, trials)
        out = np.empty((clusters, trials, 8), dtype=np.float64)
        self._check(self.lib.mh_compat_trial_stats(self._h, _p(pts, C.c_double), _p(begin, C.c_int), clusters, _p(tri, C.c_int),
                                                   _p(H, C.c_double), _p(ok, C.c_ubyte), trials, _p(out, C.c_double)))
        return out

    def compat_trial_stats_fit(self, pts_xyxy, cluster_begin, tri, F):
        """mh_compat_trial_stats_fit: the trials' 3-point homographies fitted on the device.  Returns (stats [clusters, trials, 8],
        H [clusters, trials, 9], ok [clusters, trials])."""
        pts = _f64(pts_xyxy).reshape(-1, 4)
        begin = np.ascontiguousarray(cluster_begin, dtype=np.int32)
        tri = np.ascontiguousarray(tri, dtype=np.int32)
        clusters, trials = tri.shape[0], tri.shape[1]
        F = _f64(F).reshape(9)
        out = np.empty((clusters, trials, 8), dtype=np.float64)
        H = np.empty((clusters, trials, 9), dtype=np.float64)
        ok = np.empty((clusters, trials), dtype=np.uint8)
        self._check(self.lib.mh_compat_trial_stats_fit(self._h, _p(pts, C.c_double), _p(begin, C.c_int), clusters, _p(tri, C.c_int),
                                                       _p(F, C.c_double), trials, _p(out, C.c_double), _p(H, C.c_double), _p(ok, C.c_ubyte)))
        return out, H, ok

    def compat_dlt_medians(self, pts_xyxy, cluster_begin, seed: int, first: int, trials: int):
        """mh_compat_dlt_medians: the compatibility check without F.  Per cluster `trials` 4-point DLT fits to random members,
        each trial's lower median of the other members' forward transfer errors, and the lower median of those.  Returns
        (medians [clusters], trial values [clusters, trials], H [clusters, trials, 9], idx int32 [clusters, trials, 4] —
        positions in the concatenated points)."""
        pts = _f64(pts_xyxy).reshape(-1, 4)
        begin = np.ascontiguousarray(cluster_begin, dtype=np.int32).reshape(-1)
        clusters, trials = begin.size - 1, int(trials)
        shape = (max(clusters, 0), max(trials, 0))
        med = np.empty(shape[0], dtype=np.float64)
        val = np.empty(shape, dtype=np.float64)
        H = np.empty(shape + (9,), dtype=np.float64)
        idx = np.empty(shape + (4,), dtype=np.int32)
        self._check(self.lib.mh_compat_dlt_medians(self._h, _p(pts, C.c_double), _p(begin, C.c_int), clusters, C.c_ulonglong(seed),
                                                   C.c_longlong(first), trials, _p(med, C.c_double), _p(val, C.c_double),
                                                   _p(H, C.c_double), _p(idx, C.c_int)))
        return med, val, H, idx

    def expand_stats(self):
        st = (C.c_longlong * 24)()
        self._check(self.lib.mh_get_expand_stats(self._h, st))
        return dict(zip(("cycles", "moves", "accepted", "push_phases", "relax_intervals", "host_syncs",
                         "reduce_launches", "flow_moves", "launches", "moves_run", "moves_solved",
                         "core_sites", "core_max", "barriers", "relabels", "solve_us", "barrier_us", "relax_us", "push_us", "tail_us",
                         "barrier_timeout_retries", "solver_workgroups", "xcd_local_moves", "longest_barrier_wait_us"),
                        list(st)))

    def expand_batch_stats(self):
        st = (C.c_longlong * 8)()
        self._check(self.lib.mh_get_expand_batch_stats(self._h, st))
        return dict(zip(("batches", "batch_committed", "batch_invalid", "host_skipped", "solo_moves", "injected_discarded", "moves_per_batch",
                         "batch_min_labels"), list(st)))

    def expand_trace(self, moves: int):
        out = np.zeros((int(moves), 8), dtype=np.int32)
        self._check(self.lib.mh_get_expand_trace(self._h, _p(out, C.c_int), int(moves)))
        return out

    def core_components(self, moves: int):
        out = np.zeros((int(moves), 16), dtype=np.int32)
        self._check(self.lib.mh_get_core_components(self._h, _p(out, C.c_int), int(moves)))
        return out

    def set_estimator(self, name: str):
        """mh_set_estimator: "haf" (default), "3pt" (point-only least squares with F) or "dlt" (N-point DLT, no F)."""
        if name not in ESTIMATORS:
            raise ValueError(f"unknown estimator {name!r} (haf | 3pt | dlt)")
        self._check(self.lib.mh_set_estimator(self._h, ESTIMATORS[name]))

    def set_estimator_reweighting(self, rounds: int, c2: float = 0.0):
        """mh_set_estimator_reweighting: under the "dlt" estimator, mh_reestimate and mh_labeling_step run `rounds` reweighted
        rounds at scale c2 from each label's standing model instead of the plain fit; 0 (default) off.  Sticky."""
        self._check(self.lib.mh_set_estimator_reweighting(self._h, int(rounds), C.c_double(c2)))

    def set_estimator_reweighting_auto(self, rounds: int, num: int = 1, den: int = 2, kappa2: float = 1.0, c2_min: float = 1.0,
                                       c2_max: float = 1.0):
        """mh_set_estimator_reweighting_auto: as set_estimator_reweighting with the scale of every round taken from the label's
        own errors (reweight_homographies_auto's rule); replaces the fixed rule, and set_estimator_reweighting replaces this
        one; 0 rounds off.  Sticky."""
        self._check(self.lib.mh_set_estimator_reweighting_auto(self._h, int(rounds), int(num), int(den), C.c_double(kappa2),
                                                               C.c_double(c2_min), C.c_double(c2_max)))

    def set_data_term(self, name: str):
        """mh_set_data_term: "reference" (default) or "rising" (the cost grows with the error); sticky, marks the data cost stale."""
        if name not in DATA_TERMS:
            raise ValueError(f"unknown data term {name!r} (reference | rising)")
        self._check(self.lib.mh_set_data_term(self._h, DATA_TERMS[name]))

    def reestimate(self, labels):
        labels = _i32(labels)
        H = np.empty((self.model_count, 9), dtype=np.float64)
        self._check(self.lib.mh_reestimate(self._h, _p(labels, C.c_int), _p(H, C.c_double)))
        return H

    def labeling_step(self, warm: bool, labeling):
        lab = _i32(labeling).copy()
        energy, cycles = C.c_double(0), C.c_int(0)
        self._check(self.lib.mh_labeling_step(self._h, int(bool(warm)), _p(lab, C.c_int), C.byref(energy),
                                              C.byref(cycles)))
        return lab, energy.value, cycles.value

    def merge_deltas(self, labels, pairs, H_out=None):
        """mh_merge_deltas: per pair (a, b) of labels the N-point fit of the union, the energy change `delta` of relabelling
        b -> a with that fit as model a, parts = (|S|, data_old, data_new, cut) and status (MERGE_OK / MERGE_EMPTY /
        MERGE_NO_FIT).  A pair that is not OK has delta = MERGE_NO_DELTA and keeps its rows of H_out / parts (zeros when no
        H_out is given).  Returns (H [npairs, 9], delta int64, parts int64 [npairs, 4], status int32)."""
        labels = _i32(labels)
        pairs = _i32(pairs).reshape(-1, 2)
        npairs = pairs.shape[0]
        H = np.zeros((npairs, 9), dtype=np.float64) if H_out is None else H_out
        if H.dtype != np.float64 or H.shape != (npairs, 9) or not H.flags.c_contiguous:
            raise ValueError("H_out must be a C-contiguous float64 array of shape (npairs, 9)")
        delta = np.zeros(npairs, dtype=np.int64)
        parts = np.zeros((npairs, 4), dtype=np.int64)
        status = np.zeros(npairs, dtype=np.int32)
        self._check(self.lib.mh_merge_deltas(self._h, _p(labels, C.c_int), _p(pairs, C.c_int), npairs, _p(H, C.c_double),
                                             _p(delta, C.c_longlong), _p(parts, C.c_longlong), _p(status, C.c_int)))
        return H, delta, parts, status

    def labeling_energy(self, labels):
        """mh_labeling_energy: (energy, data, smooth) of the labeling (-1..Nh-1 per point) under the resident models."""
        labels = _i32(labels)
        energy, parts = C.c_longlong(0), (C.c_longlong * 2)()
        self._check(self.lib.mh_labeling_energy(self._h, _p(labels, C.c_int), C.byref(energy), parts))
        return int(energy.value), int(parts[0]), int(parts[1])

    def best_alternative(self, labels):
        """mh_best_alternative: per point the cheapest label other than its own among the outlier label and the used labels
        (the outlier first, then the lowest index), that cost and the cost under its own label.  Returns (alt, alt_cost,
        own_cost), int32 each."""
        labels = _i32(labels)
        alt, alt_cost, own_cost = (np.zeros(labels.size, dtype=np.int32) for _ in range(3))
        self._check(self.lib.mh_best_alternative(self._h, _p(labels, C.c_int), _p(alt, C.c_int), _p(alt_cost, C.c_int),
                                                 _p(own_cost, C.c_int)))
        return alt, alt_cost, own_cost

    def drop_deltas(self, labels, cand):
        """mh_drop_deltas: per candidate label k the energy change `delta` of giving each of its members its best alternative,
        parts = (|S_k|, data_old, data_new, smooth_old, smooth_new) and status (DROP_OK / DROP_EMPTY).  A candidate that is not
        OK has delta = DROP_NO_DELTA and a zero row of parts.  Returns (delta int64, parts int64 [ncand, 5], status int32, alt
        int32 [n])."""
        labels = _i32(labels)
        cand = _i32(cand).reshape(-1)
        ncand = cand.size
        delta = np.zeros(ncand, dtype=np.int64)
        parts = np.zeros((ncand, 5), dtype=np.int64)
        status = np.zeros(ncand, dtype=np.int32)
        alt = np.zeros(labels.size, dtype=np.int32)
        self._check(self.lib.mh_drop_deltas(self._h, _p(labels, C.c_int), _p(cand, C.c_int), ncand, _p(delta, C.c_longlong),
                                            _p(parts, C.c_longlong), _p(status, C.c_int), _p(alt, C.c_int)))
        return delta, parts, status, alt

    # -- device access / profiling -----------------------------------------
    def device_buffer(self, which: int):
        ptr, nbytes = C.c_void_p(), C.c_ulonglong(0)
        self._check(self.lib.mh_device_buffer(self._h, int(which), C.byref(ptr), C.byref(nbytes)))
        return ptr.value, nbytes.value

    def label_counts(self):
        """MH_BUF_LABEL_COUNTS on the host: per label its member count in the last re-estimation (mh_reestimate /
        mh_labeling_step), one int32 per model.  Copied by the HIP runtime the engine itself has loaded (a second runtime
        client in the process, such as torch, is not needed and not started)."""
        ptr, nbytes = self.device_buffer(6)
        m = self.model_count
        if not ptr or nbytes < 4 * m:
            raise MultiHError(-4, "no label counts: no re-estimation has run on this model set")
        hip = C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemcpy.restype = C.c_int
        out = np.empty(m, dtype=np.int32)
        self.synchronize()
        rc = hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), 4 * m, 2)      # hipMemcpyDeviceToHost
        if rc != 0:
            raise MultiHError(-3, f"hipMemcpy of the label counts failed ({rc})")
        return out

    def profile_enable(self, on: bool = True):
        self._check(self.lib.mh_profile_enable(self._h, int(bool(on))))

    def profile_reset(self):
        self._check(self.lib.mh_profile_reset(self._h))

    def profile_get(self, kernel: int):
        n, ms = C.c_int(0), C.c_double(0)
        self._check(self.lib.mh_profile_get(self._h, int(kernel), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def set_tuning(self, key: int, value: int):
        self._check(self.lib.mh_set_tuning(self._h, int(key), int(value)))


def device_count() -> int:
    return int(load_library().mh_device_count())
