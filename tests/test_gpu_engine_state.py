"""The engine object itself (csrc/capi_engine.hpp): whichever entry point installs a model set leaves exactly the state a fresh
engine has after the same call — nothing of the set it replaced —, and engines are created and destroyed, with work and
resources of every kind still pending, without disturbing each other or the next one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR2 = 6.25
_cache = {}


def _scene(mh, n):
    if n not in _cache:
        _cache[n] = mh.synth.make_scene(n, 3, seed=77, with_neighbours=False)
    return _cache[n]


def _engine(mh, sc):
    e = mh.Engine(device=0, thr_fund_mat=2.6, thr_hom=2.2, locality=0.005, lam=0.5, min_inliers=20)
    e.set_correspondences(sc.src, sc.dst, sc.aff)
    e.set_epipolar(sc.F, sc.e2)
    e.build_sample_neighbours(8)
    e.build_neighbors_knn(5)
    return e


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _prefetch_and_adopt(e):
    e.prefetch_dlt4(31, 0, 64)
    e.adopt_prefetched()


def _installers(sc):
    given = np.ascontiguousarray(np.concatenate([sc.H_true, sc.H_true[::-1] * 1.5, sc.H_true[:1] * 0.5])[:7])
    assert given.shape == (7, 9)
    return [
        ("propose_dlt4", lambda e: e.propose_dlt4(31, 0, 64)),
        ("set_models(7)", lambda e: e.set_models(given)),
        ("set_models(none)", lambda e: e.set_models(np.zeros((0, 9)))),
        ("adopt_prefetched", _prefetch_and_adopt),
        ("propose_haf(64, 8)", lambda e: e.propose_haf(0, 64, 1, 8, THR2)),
        ("propose_haf(0, 8)", lambda e: e.propose_haf(0, 0, 1, 8, THR2)),
        ("propose_3pt(64)", lambda e: e.propose_3pt(31, 0, 64)),
        ("propose_3pt(0)", lambda e: e.propose_3pt(31, 0, 0)),
    ]


def _observe(mh, e):
    """Everything the resident set answers for, each as arrays or as the error code; the score last (it changes the state)."""
    def ask(fn):
        try:
            r = fn()
        except mh.MultiHError as ex:
            return ("error", ex.code)
        return tuple(np.asarray(x) for x in r) if isinstance(r, tuple) else np.asarray(r)

    seen = {"model_count": e.model_count}
    seen["get_models"] = ask(lambda: _bits(e.get_models()))
    seen["get_samples"] = ask(e.get_samples)
    seen["get_haf_support"] = ask(e.get_haf_support)
    seen["select_best (never scored)"] = ask(e.select_best)
    seen["select_best_msac"] = ask(e.select_best_msac)
    seen["expand (stale data cost)"] = ask(e.expand)
    seen["score"] = ask(lambda: e.score(THR2))
    seen["select_best (scored)"] = ask(e.select_best)
    return seen


def _same(a, b):
    if isinstance(a, tuple) and isinstance(b, tuple) and len(a) == len(b):
        return all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, tuple) or isinstance(b, tuple):
        return False
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def test_each_installer_leaves_only_its_own_state(mh, engine_lib):
    """For every ordered pair (A, B) of the eight ways to install a model set: A, then everything that can go stale (weights,
    a best-model result, a data cost), then B — and the engine answers as a fresh one that only installed B."""
    sc = _scene(mh, 300)
    installers = _installers(sc)
    fresh = {}
    for name, install in installers:
        with _engine(mh, sc) as e:
            install(e)
            fresh[name] = _observe(mh, e)
    # the cases are what they claim to be
    assert fresh["propose_dlt4"]["model_count"] == 64 and fresh["set_models(7)"]["model_count"] == 7
    assert fresh["set_models(none)"]["model_count"] == 0 and fresh["propose_haf(0, 8)"]["model_count"] == 0
    assert fresh["propose_3pt(0)"]["model_count"] == 0
    assert _same(fresh["propose_dlt4"]["get_samples"], fresh["adopt_prefetched"]["get_samples"])
    assert fresh["propose_3pt(64)"]["get_samples"].shape == (64, 4)
    assert fresh["propose_haf(64, 8)"]["get_haf_support"].shape == (64,) and fresh["propose_haf(0, 8)"]["get_haf_support"].shape == (0,)
    for name in ("propose_dlt4", "set_models(7)", "set_models(none)", "propose_3pt(0)"):
        assert fresh[name]["get_haf_support"] == ("error", -4), name
    for name, seen in fresh.items():
        assert seen["select_best (never scored)"] == ("error", -4), name
        assert seen["select_best_msac"] == ("error", -4), name
        assert seen["expand (stale data cost)"] == ("error", -4), name
        if seen["model_count"] > 0:
            assert seen["score"].shape == (seen["model_count"],) and seen["select_best (scored)"][1] == seen["score"].max(), name

    wrong = []
    for name_a, install_a in installers:
        for name_b, install_b in installers:
            with _engine(mh, sc) as e:
                install_a(e)
                if e.model_count > 0:
                    e.score_msac(THR2)
                    e.select_best()
                    e.data_cost(fetch=False)
                install_b(e)
                seen = _observe(mh, e)
            for key, want in fresh[name_b].items():
                if not _same(seen[key], want):
                    wrong.append(f"{name_a} -> {name_b}: {key}: {seen[key]!r} instead of {want!r}")
    assert not wrong, "\n".join(wrong[:20])


def _round(mh, sc, data):
    """One engine's life: every kind of owned resource at small size, then close() with work still pending."""
    out = {}
    e = _engine(mh, sc)
    try:
        modes, assign, k = e.mean_shift(data, 2.2, 5)                    # the index of the climbs, the pinned result blocks and lists
        out["mean_shift"] = (_bits(modes), assign, np.int64(k))
        e1, e2 = e.epipoles(sc.F)
        keep, refined = e.refine_correspondences(sc.F, e1, e2)
        out["refine"] = (keep, _bits(refined), e.refine_reasons())
        out["inliers_of_homography"] = e.inliers_of_homography(sc.H_true[0], THR2, 1, np.zeros(sc.n, np.int32))
        e.propose_dlt4(11, 0, 256)
        H, counters, counts, _ = e.select_greedy(THR2, 12, 8)
        out["select_greedy"] = (_bits(H), counters, counts)
        twenty = e.get_models()[:20]
        e.set_models(twenty)                                             # 21 labels: the moves run as a batch, in contexts of their own
        labels, energy, cycles = e.labeling_step(False, np.full(sc.n, -1, np.int32))
        out["labeling_step"] = (labels, np.float64(energy), np.int64(cycles), _bits(e.get_models()))
        out["batches"] = np.int64(e.expand_batch_stats()["batches"] > 0)
        e.profile_enable(True)                                           # timers nobody reads
        e.propose_dlt4(12, 0, 128)
        out["score"] = e.score(THR2)
        e.residual_matrix(THR2, fetch_R=False, fetch_counts=False)
        e.select_best(fetch=False)                                       # an exchange still pending,
        e.prefetch_dlt4(13, 0, 128)                                      # and a batch still prefetched
    finally:
        e.close()
    return out


def test_engines_come_and_go(mh, engine_lib):
    sc = _scene(mh, 600)
    rng = np.random.default_rng(3)
    centres = rng.uniform(-40, 40, size=(15, 6))
    data = np.concatenate([c + rng.normal(0, 0.2, size=(40, 6)) for c in centres])          # 600 rows
    with mh.Engine(device=0, thr_fund_mat=2.6, thr_hom=2.2, locality=0.005, lam=0.5, min_inliers=20) as other:
        other.set_correspondences(sc.src, sc.dst, sc.aff)
        other.propose_dlt4(7, 0, 200)
        counts = other.score(THR2)
        assert counts.max() > 20
        first = None
        for r in range(3):
            seen = _round(mh, sc, data)
            assert np.array_equal(other.score(THR2), counts), f"round {r}: the engine that stayed answers differently"
            if first is None:
                first = seen
                assert seen["mean_shift"][2] >= 15 and seen["batches"] == 1 and len(seen["select_greedy"][2]) >= 1
                continue
            assert seen.keys() == first.keys()
            for key in first:
                assert _same(seen[key], first[key]), f"round {r}: {key} differs from the first round's"
