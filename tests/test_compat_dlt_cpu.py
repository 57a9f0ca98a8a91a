"""CPU tests of the compatibility check without F: the twin tests/compat_dlt_numpy.py against the plain
definition (a numpy SVD DLT on the same tuples and a full sort), the grid the default limit is read from, the host rule on
hand-made medians, and the binding's symbol."""
import os

import numpy as np

import compat_dlt_numpy as T

THR_H = 2.2


def _plain_dlt(p):
    """The normalised DLT of four correspondences by numpy's SVD: Hartley normalisation, the right singular vector of the
    smallest singular value, de-normalised, unit Frobenius norm, h33 >= 0."""
    def norm(q):
        c = q.mean(axis=0)
        s = np.sqrt(2.0) / np.sqrt(((q - c) ** 2).sum(axis=1)).mean()
        return (q - c) * s, np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    a, T1 = norm(p[:, :2])
    b, T2 = norm(p[:, 2:])
    rows = []
    for (x, y), (u, v) in zip(a, b):
        rows.append([-x, -y, -1, 0, 0, 0, u * x, u * y, u])
        rows.append([0, 0, 0, -x, -y, -1, v * x, v * y, v])
    h = np.linalg.svd(np.array(rows))[2][-1].reshape(3, 3)
    H = np.linalg.inv(T2) @ h @ T1
    H = H / np.linalg.norm(H)
    return (H if H[2, 2] >= 0 else -H).reshape(9)


def _plain_d2(p, H):
    q = np.concatenate([p[:, :2], np.ones((p.shape[0], 1))], axis=1) @ H.reshape(3, 3).T
    return ((p[:, 2:] - q[:, :2] / q[:, 2:3]) ** 2).sum(axis=1)


def test_the_twin_equals_the_plain_definition(mh):
    sizes = (5, 19, 64, 400)
    sc = mh.synth.make_scene(2000, 3, seed=17, noise=0.6, outlier_frac=0.3, with_neighbours=False)
    pts = np.concatenate([sc.src, sc.dst], axis=1)[:sum(sizes)].copy()
    begin = np.concatenate([[0], np.cumsum(sizes)])
    trials = 25
    med, val, H, idx, wit = T.medians(pts, begin, 31, 7, trials)
    good = wit > 1e-6
    print(f"witness <= 1e-6 leaves out {int((~good).sum())} of {good.size} tuples")
    assert good.sum() > 0.5 * good.size
    worst = 0.0
    for c in range(len(sizes)):
        p = pts[begin[c]:begin[c + 1]]
        for t in range(trials):
            local = idx[c, t] - begin[c]
            assert local.min() >= 0 and local.max() < sizes[c] and len(set(local.tolist())) == 4
            if not good[c, t]:
                continue
            d = np.sort(np.delete(_plain_d2(p, _plain_dlt(p[local])), local))
            want = d[(d.size - 1) // 2]
            worst = max(worst, abs(val[c, t] - want) / want)
    print(f"largest relative difference of a trial value: {worst:.3e}")
    assert worst <= 1e-6
    assert np.array_equal(med, np.sort(val, axis=1)[:, (trials - 1) // 2])


def test_the_default_limit_is_the_grids_largest_clean_ratio_rounded_up(mh):
    """A = the largest statistic / sigma^2 over the clean grid (members x noise x perspective on the whole image,
    members x noise on a third of it, each cell once per draw), rounded up to the next power of two; the contaminated clusters
    exceed A thr_hom^2 at thr_hom = 2.2 at least twice over."""
    rows = T.clean_grid()
    assert len(rows) == len(T.GRID_DRAWS) * (len(T.GRID_MEMBERS) * len(T.GRID_SIGMA) * (len(T.GRID_PERSPECTIVE) + 1))
    ratios = np.array([r[5] for r in rows])
    worst = rows[int(ratios.argmax())]
    print(f"clean ratio statistic / sigma^2: min {ratios.min():.1f}, median {np.median(ratios):.1f}, max {ratios.max():.1f} at {worst[:5]}")
    A = T.LIMIT_SCALE
    assert A == 2.0 ** np.ceil(np.log2(ratios.max())), (A, ratios.max())
    limit = A * THR_H ** 2
    for name, stat in T.contaminated_grid():
        print(f"{name}: {stat:.4g} px^2 = {stat / limit:.1f} x the limit {limit:.0f}")
        assert stat >= 2.0 * limit, name
    # the class's default is this A
    text = open(os.path.join(os.path.dirname(mh.LIB_PATH), "host", "MultiH.h")).read()
    assert f"COMPAT_DLT_LIMIT_SCALE = {A:.1f};" in text


def test_the_host_rule_on_hand_made_medians():
    sizes = (30, 3, 25, 4, 6, 40, 5)
    labels = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)] + [np.full(9, -1)]).astype(np.int32)
    np.random.default_rng(1).shuffle(labels)
    H = np.arange(len(sizes) * 9, dtype=np.float64).reshape(-1, 9)
    seen = []

    def stat_of(values):
        def fn(clusters):
            seen.append(list(clusters))
            return [values[c] for c in clusters]
        return fn

    # min_inliers 5: 3 and 4 members go by size; 25 members go by the statistic, +inf goes, the limit itself stays
    values = {0: 10.0, 2: 10.000001, 4: 1.0, 5: np.inf, 6: 0.0}
    out, Hk, med, removed = T.host_rule(labels, H, 10.0, 5, stat_of(values))
    assert seen[-1] == [0, 2, 4, 5, 6]
    assert removed.tolist() == [False, True, True, True, False, True, False]
    assert np.array_equal(Hk, H[[0, 4, 6]])
    assert np.isnan(med[[1, 3]]).all() and med[[0, 2, 4, 5, 6]].tolist() == [10.0, 10.000001, 1.0, np.inf, 0.0]
    new = {0: 0, 4: 1, 6: 2}
    assert np.array_equal(out, np.array([new.get(int(l), -1) for l in labels]))
    # min_inliers 0: nobody goes by size; clusters of fewer than 5 members are kept without a statistic
    out, Hk, med, removed = T.host_rule(labels, H, 10.0, 0, stat_of(values))
    assert seen[-1] == [0, 2, 4, 5, 6] and removed.tolist() == [False, False, True, False, False, True, False]
    assert np.isnan(med[[1, 3]]).all() and np.array_equal(Hk, H[[0, 1, 3, 4, 6]])
    new = {0: 0, 1: 1, 3: 2, 4: 3, 6: 4}
    assert np.array_equal(out, np.array([new.get(int(l), -1) for l in labels]))
    # min_inliers 20: the clusters of 5 and 6 go by size and get no statistic
    out, Hk, med, removed = T.host_rule(labels, H, 10.0, 20, stat_of(values))
    assert seen[-1] == [0, 2, 5] and removed.tolist() == [False, True, True, True, True, True, True] and Hk.shape[0] == 1
    # nothing to pack: the statistics are not asked for
    n = len(seen)
    out, Hk, med, removed = T.host_rule(np.zeros(4, np.int32), H[:1], 10.0, 0, stat_of(values))
    assert len(seen) == n and not removed.any() and np.isnan(med).all() and np.array_equal(out, np.zeros(4))


def test_check_packs_in_cluster_order_with_first_zero(mh):
    sc = mh.synth.make_scene(600, 3, seed=5, noise=0.4, outlier_frac=0.2, with_neighbours=False)
    labels = sc.gt_label.copy()
    calls = []

    def medians_of(pts, begin, seed, first, trials):
        calls.append((pts.copy(), np.array(begin), seed, first, trials))
        return T.medians(pts, begin, seed, first, trials)[0]
    out, Hk, med, removed = T.check(sc.src, sc.dst, labels, sc.H_true, 256 * THR_H ** 2, 20, 4242, 51, medians_of)
    pts, begin, seed, first, trials = calls[0]
    assert (seed, first, trials) == (4242, 0, 51) and begin[0] == 0
    for q in range(3):
        own = labels == q
        assert np.array_equal(pts[begin[q]:begin[q + 1]], np.concatenate([sc.src[own], sc.dst[own]], axis=1))
    assert not removed.any() and np.array_equal(out, labels) and np.isfinite(med).all()


def test_the_binding_names_the_entry_point(mh, engine_lib):
    assert "mh_compat_dlt_medians" in mh.SYMBOLS and hasattr(engine_lib, "mh_compat_dlt_medians")
    assert callable(mh.Engine.compat_dlt_medians)


def test_the_harness_checks_its_flag(mh, engine_lib, tmp_path):
    import subprocess
    harness = os.path.join(os.path.dirname(mh.LIB_PATH), "multih_harness")
    missing = str(tmp_path / "no_such_file.txt")
    for value, status in (("dlt:0", 2), ("dlt:4097", 2), ("dlt:100:0", 2), ("dlt:100:x", 2), ("3pt", 2), ("dlt", 1), ("dlt:100:64", 1)):
        r = subprocess.run([harness, missing, str(tmp_path / "out.txt"), "--compat-fit", value], capture_output=True, text=True, timeout=60)
        assert r.returncode == status, (value, r.stderr[-300:])               # (1: the flag passed, the input file is missing)
        assert ("--compat-fit: dlt[:trials[:limit_scale]]" in r.stderr) == (status == 2)
