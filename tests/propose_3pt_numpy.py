"""A twin of the 3-point proposer (include/multih_hip.h, mh_propose_3pt), from the CPU alone.

Hypothesis s of a batch has counter c = first + s.  Its tuple is the first three indices of the 4-tuple the proposer's sampler
gives that counter — oracle_lib.sample4 under the uniform sampler, local_sampler_numpy.sample_local under the local one — and
its model is GetHomography3PT without refinement on those three correspondences and F, computed by the host library's
Homography3PTLinear (libmultih_host.so, mhh_homography_3pt: plain C++ on the CPU, the yardstick tests/test_gpu_postfilter.py
holds the device's fit to).  A fit that fails is nine quiet NaNs."""
import ctypes as C
import os

import numpy as np

import local_sampler_numpy as L
import oracle_lib as O

knn_table = L.knn_table
_dp = C.POINTER(C.c_double)
_host = {}


def host_lib(lib_path):
    """libmultih_host.so next to the engine library `lib_path`."""
    path = os.path.join(os.path.dirname(lib_path), "libmultih_host.so")
    if path not in _host:
        _host[path] = C.CDLL(path)
    return _host[path]


def tuples(seed, first, m, n, nbr=None, uniform_per_16=0):
    """m x 3: the tuples of counters first .. first + m - 1; nbr: the sampling table of the local sampler, None = uniform."""
    if m == 0:
        return np.zeros((0, 3), dtype=np.int32)
    idx = O.sample4(seed, first, m, n) if nbr is None else L.sample_local(seed, first, m, n, nbr, uniform_per_16)
    return np.ascontiguousarray(idx[:, :3])


def samples(idx3):
    """What mh_get_samples returns for the batch: the three indices and -1 in the fourth column."""
    return np.concatenate([idx3, np.full((idx3.shape[0], 1), -1, dtype=np.int32)], axis=1).astype(np.int32)


def fit(host, src, dst, F, idx3):
    """(H [m, 9], ok [m]): the host's fit of every tuple; rows whose fit fails are all NaN."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.float64).reshape(9)
    m = idx3.shape[0]
    H = np.full((m, 9), np.nan)
    ok = np.zeros(m, dtype=bool)
    h = np.zeros(9)
    for s in range(m):
        p1, p2 = np.ascontiguousarray(src[idx3[s]]), np.ascontiguousarray(dst[idx3[s]])
        ok[s] = host.mhh_homography_3pt(p1.ctypes.data_as(_dp), p2.ctypes.data_as(_dp), 3, F.ctypes.data_as(_dp), h.ctypes.data_as(_dp)) == 1
        if ok[s]:
            H[s] = h
    return H, ok


def propose(host, src, dst, F, seed, first, m, nbr=None, uniform_per_16=0):
    """(H [m, 9], samples [m, 4]) of mh_propose_3pt(seed, first, m) on these correspondences."""
    idx3 = tuples(seed, first, m, np.asarray(src).shape[0], nbr, uniform_per_16)
    return fit(host, src, dst, F, idx3)[0], samples(idx3)
