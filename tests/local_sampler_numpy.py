"""numpy twin of the neighbourhood-guided proposal sampler (csrc/dlt4.hip, sample4_by; include/multih_hip.h, mh_set_sampler)
and of its table (mh_build_sample_neighbours).  Written from the rule, not from the kernel:

  draw j of hypothesis c:  r_j = splitmix64(seed + (c << 8) + j), everything modulo 2^64
  index from a draw:       ((r >> 32) * range) >> 32
  uniform tuple:           draws 0 .. 63 over N, a draw taken unless its index is already in the tuple, until there are four;
                           empty slots take the first index
  local tuple:             (c & 15) < uniform_per_16: the uniform tuple.  Otherwise i0 = the index of draw 0 over N; draws
                           1 .. 63 index row i0 of the table (range k), a candidate taken unless it is already in the tuple, until
                           there are four; empty slots take i0
  table:                   row i = the k indices j != i with the smallest (d(i, j), j), d the float32 squared distance in
                           (x1, y1, x2, y2): ((dx dx + dy dy) + dz dz) + dw dw, every operation rounded to float32
"""
import numpy as np

MASK = (1 << 64) - 1


def splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _draw(seed: int, c: int, j: int, rng: int) -> int:
    r = splitmix64((seed + ((c << 8) & MASK) + j) & MASK)
    return ((r >> 32) * rng) >> 32


def uniform_tuple(seed: int, c: int, n: int) -> list:
    out = []
    for j in range(64):
        if len(out) == 4:
            break
        i = _draw(seed, c, j, n)
        if i not in out:
            out.append(i)
    return out + [out[0]] * (4 - len(out))


def local_tuple(seed: int, c: int, n: int, nbr: np.ndarray, uniform_per_16: int) -> list:
    if (c & 15) < uniform_per_16:
        return uniform_tuple(seed, c, n)
    k = nbr.shape[1]
    out = [_draw(seed, c, 0, n)]
    row = nbr[out[0]]
    for j in range(1, 64):
        if len(out) == 4:
            break
        cand = int(row[_draw(seed, c, j, k)])
        if cand not in out:
            out.append(cand)
    return out + [out[0]] * (4 - len(out))


def sample_local(seed: int, first: int, m: int, n: int, nbr: np.ndarray, uniform_per_16: int) -> np.ndarray:
    """The m tuples of counters first .. first + m - 1 (first: the signed 64-bit counter of the C interface)."""
    seed &= MASK
    return np.array([local_tuple(seed, (first + s) & MASK, n, nbr, uniform_per_16) for s in range(m)], dtype=np.int32).reshape(m, 4)


def sample_uniform(seed: int, first: int, m: int, n: int) -> np.ndarray:
    seed &= MASK
    return np.array([uniform_tuple(seed, (first + s) & MASK, n) for s in range(m)], dtype=np.int32).reshape(m, 4)


def knn_table(src: np.ndarray, dst: np.ndarray, k: int) -> np.ndarray:
    """Brute force: float32 distances, a stable sort on d over j ascending = the order (d, j)."""
    P = np.concatenate([src, dst], axis=1).astype(np.float32)
    n = P.shape[0]
    assert 0 < k < n
    out = np.empty((n, k), dtype=np.int32)
    for i in range(n):
        df = P[i][None, :] - P
        d = ((df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2]) + df[:, 3] * df[:, 3]
        assert d.dtype == np.float32
        order = np.argsort(d, kind="stable")
        order = order[order != i]
        out[i] = order[:k]
    return out


def same_plane_share(idx: np.ndarray, gt_label: np.ndarray) -> float:
    """Share of tuples whose four indices are distinct and all on one true plane (label >= 0)."""
    lab = gt_label[idx]
    distinct = np.array([len(set(t)) == 4 for t in idx.tolist()])
    one = (lab >= 0).all(axis=1) & (lab == lab[:, :1]).all(axis=1)
    return float(np.mean(distinct & one))
