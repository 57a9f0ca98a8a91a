"""mh_compat_dlt_medians (include/multih_hip.h; csrc/compat.hip, k_compat_median4 and k_compat_cluster_median over the fits of
k_dlt4's segment sampler) and multih::CompatibilityCheckDlt (host/merge_step.cpp) in numpy: the TWIN of the compatibility check
without F.

    tuples        per cluster the trials' four local positions: oracle_lib.sample4(seed, first + c * trials, trials, nc)
    medians       tuples -> oracle_lib.dlt4 -> keys from oracle_lib.residual_matrix (NaN counts as +inf) -> the key at rank
                  (rest - 1) // 2 of the members that are none of the tuple's four -> per cluster the value at rank
                  (trials - 1) // 2 of its trial values.  Ranks are taken by sorting.
    host_rule     which clusters go: fewer than min_inliers members -> removed; at least max(min_inliers, 5) -> a statistic,
                  removed if and only if it exceeds the limit; otherwise kept without one (its median is NaN).  Labels are
                  renumbered and H compacted as by multih::CompatibilityCheck.
    check         host_rule with the statistics of `medians` over the clusters packed in cluster order, first = 0.
    clean_plane, two_planes, scrambled   the scenes of the limit's grid.
"""
import numpy as np

import oracle_lib as O

MIN_POINTS = 5
IMG = 1000.0


def tuples(seed, first, trials, sizes):
    """Per cluster c an int32 array [trials, 4] of local positions (counter first + c * trials + t)."""
    return [O.sample4(seed, first + c * trials, trials, int(nc)) for c, nc in enumerate(sizes)]


def trial_values(p, tup, H):
    """p [nc, 4], tup [T, 4] local positions, H [T, 9] -> [T]: the lower median of the others' forward errors, by sorting."""
    nc = p.shape[0]
    with np.errstate(all="ignore"):
        R = O.residual_matrix(p[:, :2], p[:, 2:], H)                        # T x nc, the engine's formula bit for bit
    R = np.where(np.isnan(R), np.inf, R)
    out = np.empty(tup.shape[0])
    for t in range(tup.shape[0]):
        keep = np.ones(nc, dtype=bool)
        keep[tup[t]] = False
        d = np.sort(R[t][keep])
        out[t] = d[(d.size - 1) // 2]
    return out


def medians(pts_xyxy, begin, seed, first, trials, H=None):
    """(medians [C], trial values [C, T], H [C, T, 9], idx [C, T, 4] global positions, witness [C, T]).  H given: the fits are
    taken from it (the engine's own), the tuples still from the rule."""
    pts = np.ascontiguousarray(pts_xyxy, dtype=np.float64).reshape(-1, 4)
    begin = np.asarray(begin, dtype=np.int64)
    C = begin.size - 1
    sizes = np.diff(begin)
    tup = tuples(seed, first, trials, sizes)
    idx = np.stack([tup[c] + begin[c] for c in range(C)]).astype(np.int32)
    with np.errstate(all="ignore"):
        H_o, wit, _ = O.dlt4(pts[:, :2], pts[:, 2:], idx.reshape(-1, 4))
    H_o, wit = H_o.reshape(C, trials, 9), wit.reshape(C, trials)
    Hs = H_o if H is None else np.asarray(H, dtype=np.float64).reshape(C, trials, 9)
    val = np.stack([trial_values(pts[begin[c]:begin[c + 1]], tup[c], Hs[c]) for c in range(C)])
    med = np.sort(val, axis=1)[:, (trials - 1) // 2]
    return med, val, Hs, idx, wit


def host_rule(labels, H, limit, min_inliers, stat_of):
    """labels [n] in -1 .. nh-1, H [nh, 9].  stat_of(list of clusters that get a statistic, in cluster order) -> their statistics.
    Returns (labels_out, H_out [kept, 9], medians [nh] — NaN where the cluster got none —, removed [nh] bool)."""
    labels = np.array(labels, dtype=np.int32)
    H = np.array(H, dtype=np.float64).reshape(-1, 9)
    nh = H.shape[0]
    sizes = np.array([(labels == c).sum() for c in range(nh)])
    remove = sizes < min_inliers
    stat = [c for c in range(nh) if sizes[c] >= max(min_inliers, MIN_POINTS)]
    med = np.full(nh, np.nan)
    if stat:
        med[stat] = np.asarray(stat_of(stat), dtype=np.float64)
        remove[stat] = med[stat] > limit
    new = np.full(nh, -1, dtype=np.int32)
    new[~remove] = np.arange(int((~remove).sum()), dtype=np.int32)
    out = labels.copy()
    own = (labels >= 0) & (labels < nh)
    out[own] = new[labels[own]]
    return out, H[~remove].copy(), med, remove


def pack(src, dst, labels, clusters):
    """The clusters' points back to back in point order, and cluster_begin."""
    parts = [np.concatenate([src[labels == c], dst[labels == c]], axis=1) for c in clusters]
    begin = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(parts)), begin


def check(src, dst, labels, H, limit, min_inliers, seed, trials, medians_of=None):
    """multih::CompatibilityCheckDlt.  medians_of(pts, begin, seed, first, trials) -> medians (default: the twin's)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    labels = np.asarray(labels)
    fn = medians_of or (lambda p, b, s, f, t: medians(p, b, s, f, t)[0])

    def stat_of(clusters):
        pts, begin = pack(src, dst, labels, clusters)
        return fn(pts, begin, seed, 0, trials)
    return host_rule(labels, H, limit, min_inliers, stat_of)


# ---- the scenes of the limit's grid -------------------------------------------------------------------------------------

def _apply(H, p):
    q = np.concatenate([p, np.ones((p.shape[0], 1))], axis=1) @ np.asarray(H).reshape(3, 3).T
    return q[:, :2] / q[:, 2:3]


def draw_h(rng, perspective):
    """A homography of a 1000 px image: an affine part near the identity, a shift of up to 40 px, and a third row of the given
    size (perspective * 1000 is the relative change of the denominator across the image)."""
    H = np.eye(3)
    H[:2, :2] += rng.normal(0, 0.08, size=(2, 2))
    H[:2, 2] = rng.uniform(-40, 40, size=2)
    v = rng.normal(size=2)
    H[2, :2] = perspective * v / np.linalg.norm(v)
    return H


def clean_plane(n, sigma, perspective, rng, third=False):
    """n correspondences of one plane, `sigma` px of Gaussian noise per axis on the targets (as synth.make_scene and
    three_motions place it: the forward transfer error of an inlier is then that noise); third: the plane covers a third of the
    image's width.  Returns pts [n, 4]."""
    H = draw_h(rng, perspective)
    src = rng.uniform(0.0, IMG, size=(n, 2))
    if third:
        src[:, 0] /= 3.0
    dst = _apply(H, src) + rng.normal(0, sigma, size=(n, 2))
    return np.concatenate([src, dst], axis=1)


def two_planes(n, share, sigma, rng):
    """A cluster of two planes: `share` of the members on the second one."""
    a = clean_plane(n, sigma, 5e-5, rng)
    k = int(round(share * n))
    H2 = draw_h(rng, 5e-5)
    a[:k, 2:] = _apply(H2, a[:k, :2]) + rng.normal(0, sigma, size=(k, 2))
    return a


def scrambled(n, share, sigma, rng):
    """A plane of which `share` of the members have a random destination."""
    a = clean_plane(n, sigma, 5e-5, rng)
    k = int(round(share * n))
    a[:k, 2:] = rng.uniform(0.0, IMG, size=(k, 2))
    return a


GRID_MEMBERS = (19, 64, 400, 2000)
GRID_SIGMA = (0.3, 0.5, 1.0)
GRID_PERSPECTIVE = (0.0, 5e-5, 2e-4)
GRID_TRIALS = 501
GRID_DRAWS = (20, 1, 2, 3)  # every cell is drawn once per seed: the statistic of a clean plane spreads by about 2x from scene to scene
LIMIT_SCALE = 256.0         # A of DESIGN.md 3.17: the largest clean ratio of the grid, rounded up to a power of two


def clean_grid(draws=GRID_DRAWS):
    """[(members, sigma, perspective, third, draw, statistic / sigma^2)] over the grid: every size x noise x perspective on the
    whole image, and every size x noise at the middle perspective on a third of it, each once per draw."""
    rows = []
    cases = [(n, s, p, False) for n in GRID_MEMBERS for s in GRID_SIGMA for p in GRID_PERSPECTIVE]
    cases += [(n, s, GRID_PERSPECTIVE[1], True) for n in GRID_MEMBERS for s in GRID_SIGMA]
    for draw in draws:
        rng = np.random.default_rng(draw)
        for i, (n, s, p, third) in enumerate(cases):
            pts = clean_plane(n, s, p, rng, third)
            med = medians(pts, [0, n], 1000 + i, 0, GRID_TRIALS)[0][0]
            rows.append((n, s, p, third, draw, med / (s * s)))
    return rows


def contaminated_grid(seed=21, n=400, sigma=0.5):
    """[(name, statistic in px^2)] of the counter-cases."""
    rng = np.random.default_rng(seed)
    cases = [("two planes 50/50", two_planes(n, 0.5, sigma, rng)), ("two planes 75/25", two_planes(n, 0.25, sigma, rng)),
             ("a third scrambled", scrambled(n, 1.0 / 3.0, sigma, rng)), ("half scrambled", scrambled(n, 0.5, sigma, rng))]
    return [(name, medians(p, [0, n], 2000 + i, 0, GRID_TRIALS)[0][0]) for i, (name, p) in enumerate(cases)]
