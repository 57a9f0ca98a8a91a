"""mh_label_residual_quantile and mh_reweight_homographies_auto (include/multih_hip.h; csrc/label_scale.hip, k_label_quantile and
k_autoscale_reweight_h) in numpy: the TWIN of the rules in the header, so that the kernels can be held to it bit for bit.

    quantile         numpy.sort of the members' keys viewed as uint64, indexed at the integer rank ((c - 1) * num) / den.  The
                     key is refit_h_numpy.d2_of (the forward transfer error in the reference's operation order), +inf for a NaN.
    reweight_auto    reweight_h_numpy's weights, wfit and gain_of with c2 = clamp(kappa2 * quantile under the model that stands)
                     re-estimated in every round.

tests/test_label_scale_cpu.py holds the twin to numpy.partition, to reweight_h_numpy.reweight where the bounds coincide, and to
what it is for; tests/test_gpu_label_scale.py holds the kernels to the twin.
"""
import numpy as np

import refit_h_numpy as R
import reweight_h_numpy as W

MAX_DEN = 65536
QNAN_BITS = np.uint64(0x7ff8000000000000)
KAPPA2_DEFAULT = 6.643856189774724                              # log2(100), the nearest double: the host's default kappa^2
assert KAPPA2_DEFAULT == float(np.log2(100.0))


def rank_of(c, num, den):
    """The 0-based rank of the order statistic among c members: ((c - 1) * num) / den by integer division."""
    assert 1 <= den <= MAX_DEN and 0 <= num <= den and c >= 1
    return ((int(c) - 1) * int(num)) // int(den)


def keys_of(src, dst, idx, H):
    """The keys of the members idx under H as float64: d2, +inf where it is a NaN."""
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size == 0:
        return np.zeros(0)
    with np.errstate(all="ignore"):
        d2 = R.d2_of(np.asarray(src, np.float64)[idx], np.asarray(dst, np.float64)[idx], H)
    d2 = np.where(np.isnan(d2), np.inf, d2)
    assert not np.any(np.signbit(d2)), "a sum of two squares: never negative, never -0"
    return np.ascontiguousarray(d2, dtype=np.float64)


def select(keys, num, den):
    """(value, rank, members strictly below the value) of the float64 keys (non-negative or +inf, at least one)."""
    bits = np.ascontiguousarray(keys, np.float64).view(np.uint64)
    r = rank_of(bits.size, num, den)
    v = np.sort(bits)[r]
    return float(np.array([v], dtype=np.uint64).view(np.float64)[0]), r, int((bits < v).sum())


def quantile_one(src, dst, idx, H, num, den):
    """One label: (d2, (members, rank, below, status))."""
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size == 0:
        return float(np.array([QNAN_BITS]).view(np.float64)[0]), (0, 0, 0, 1)
    v, r, below = select(keys_of(src, dst, idx, H), num, den)
    return v, (int(idx.size), r, below, 0)


def quantile(src, dst, labels, H, num, den):
    """The twin of mh_label_residual_quantile: (d2 [m], info int32 [m, 4])."""
    assert 1 <= den <= MAX_DEN and 0 <= num <= den
    labels = np.asarray(labels)
    H = np.array(H, dtype=np.float64).reshape(-1, 9)
    m = H.shape[0]
    d2, info = np.empty(m), np.empty((m, 4), dtype=np.int32)
    for k in range(m):
        d2[k], info[k] = quantile_one(src, dst, np.flatnonzero(labels == k), H[k], num, den)
    return d2, info


def scale_of(src, dst, idx, H, num, den, kappa2, c2_min, c2_max):
    """scale(H) of the header: one multiplication, then the clamp."""
    q = select(keys_of(src, dst, idx, H), num, den)[0]
    with np.errstate(all="ignore"):
        s = float(np.float64(kappa2) * np.float64(q))
    assert not np.isnan(s)
    return c2_min if s < c2_min else (c2_max if s > c2_max else s)


def reweight_auto_one(src, dst, idx, H_in, num, den, kappa2, c2_min, c2_max, rounds):
    """One label: (H_out[9], (W_in, W_out), (c2_in, c2_out), (members, support, done, status))."""
    H_in = np.array(H_in, dtype=np.float64).reshape(9)
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size < 4:
        return H_in.copy(), (0.0, 0.0), (0.0, 0.0), (int(idx.size), 0, 0, 1)
    if not np.all(np.isfinite(H_in)):
        return H_in.copy(), (0.0, 0.0), (0.0, 0.0), (int(idx.size), 0, 0, 2)
    scale = lambda H: scale_of(src, dst, idx, H, num, den, kappa2, c2_min, c2_max)
    cur, done = H_in.copy(), 0
    c2 = c2_in = scale(cur)
    w = W.weights(src, dst, idx, cur, c2)
    W_in = W.gain_of(idx, w)[0]
    for _ in range(rounds):
        cand = W.wfit(src, dst, idx, w)
        if cand is None or R.same_bits(cand, cur):
            break
        cur, done = cand, done + 1
        c2 = scale(cur)
        w = W.weights(src, dst, idx, cur, c2)
    W_out, support = W.gain_of(idx, w)
    return cur, (W_in, W_out), (c2_in, c2), (int(idx.size), support, done, 0)


def reweight_auto(src, dst, labels, H_in, num, den, kappa2, c2_min, c2_max, rounds):
    """The twin of mh_reweight_homographies_auto: (H_out [m, 9], gain [m, 2], scale [m, 2], info int32 [m, 4])."""
    assert 0 <= rounds <= W.MAX_ROUNDS and 1 <= den <= MAX_DEN and 0 <= num <= den
    assert np.isfinite(kappa2) and kappa2 > 0 and np.isfinite(c2_min) and np.isfinite(c2_max) and 0 < c2_min <= c2_max
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    labels = np.asarray(labels)
    H_in = np.array(H_in, dtype=np.float64).reshape(-1, 9)
    m = H_in.shape[0]
    H, gain, scale, info = np.empty((m, 9)), np.empty((m, 2)), np.empty((m, 2)), np.empty((m, 4), dtype=np.int32)
    for k in range(m):
        H[k], gain[k], scale[k], info[k] = reweight_auto_one(src, dst, np.flatnonzero(labels == k), H_in[k], num, den, kappa2,
                                                             c2_min, c2_max, rounds)
    return H, gain, scale, info


def reestimate_auto(src, dst, labels, H_in, num, den, kappa2, c2_min, c2_max, rounds):
    """MH_ESTIMATOR_DLT under mh_set_estimator_reweighting_auto, rounds >= 1: (H [Nh, 9], counts [Nh])."""
    H, _, _, info = reweight_auto(src, dst, labels, H_in, num, den, kappa2, c2_min, c2_max, rounds)
    return H, info[:, 0].copy()


# ---- the scene of the direction tests -------------------------------------------------------------------------------------

def shifted_plane(rng, sigma, contaminants, members=400):
    """`members` correspondences of one plane with Gaussian noise sigma on the targets and `contaminants` more whose targets lie
    5 sigma to ONE side (a fixed direction) with 0.6 sigma of scatter, shuffled: (src, dst, H_true[9], on_plane[n])."""
    n = members + contaminants
    src, dst, H_true, _ = R.plane_scene(rng, n, 0.0)
    ang = rng.uniform(0, 2 * np.pi)
    side = np.array([np.cos(ang), np.sin(ang)])
    on_plane = np.zeros(n, bool)
    on_plane[rng.permutation(n)[:members]] = True
    dst = dst.copy()
    dst[on_plane] += rng.normal(0, sigma, size=(members, 2))
    if contaminants:
        dst[~on_plane] += 5.0 * sigma * side + rng.normal(0, 0.6 * sigma, size=(contaminants, 2))
    return src, np.ascontiguousarray(dst), H_true, on_plane
