#!/usr/bin/env python3
"""What the per-label residual quantile and the self-scaled reweighted refits (mh_label_residual_quantile,
mh_reweight_homographies_auto, csrc/label_scale.hip; mh_set_estimator_reweighting_auto; MultiH::SetModelReweightAuto /
SetEstimatorReweightAuto) cost and buy, on one MI355X:

  kernel   kernel times by the engine's per-kernel events (mh_profile_*, the MH_K_REESTIMATE slot), the median of REPS runs
           (default 21), at 50 000 points x 11 labels and 20 000 points x 540 labels: k_label_quantile alone (the lower median),
           and mh_reestimate under "dlt" with k_reweight_h (fixed c2 = thr_hom^2) beside k_autoscale_reweight_h (the host's
           numbers) at 1 and 3 rounds.  Every run starts from the same models.  A call of r auto rounds runs r + 1 selections on
           top of the fixed call's passes: (auto - fixed) / (r + 1) is what one selection adds.
  final    Process() with the epipolar geometry given on the 20 000 / 6 and 50 000 / 10 synthetic scenes, then over the run's
           labels from its models: no refit, three fixed rounds at thr_hom (--reweight 3) and three self-scaled rounds
           (--reweight-auto 3, which tests/test_gpu_label_scale.py holds equal to the call bit for bit): per cluster the RMS
           distance between H p and H_true p over the points of the plane most of its members come from.
  barrsmith  the reference's rows of barrsmith (tools/barrsmith_agreement.py), F given, the twelve seeds of
           profiles/r06_barrsmith_agreement.txt: SetEstimator(ESTIMATOR_DLT) plain, with SetEstimatorReweight(2) and with
           SetEstimatorReweightAuto(2): planes and the ARI on the reference's inliers, median / min / max.

  python tools/label_scale_probe.py | grep -v '^\\[Multi-H\\]\\|^Iteration' > profiles/label_scale_probe.txt
Every part is a child process under a time limit of its own; nothing more is started after a part that did not end well."""
import ctypes as C
import importlib
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIMIT = 240                                        # seconds per part
REPS = int(os.environ.get("REPS", 21))
THR = 2.2
K_REESTIMATE = 5
SEEDS = (1234, 7, 99, 1, 2, 3, 4, 5, 6, 8, 9, 10)
KAPPA2 = 6.643856189774724                         # log2(100): the host's default
DBL_MIN = 2.2250738585072014e-308
C2_MAX = THR * THR * 81.0 / 16.0
AUTO = (1, 2, KAPPA2, DBL_MIN, C2_MAX)


def _host(mh):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    for fn in (host.mhh_set_estimator_reweight, host.mhh_set_estimator_reweight_auto, host.mhh_set_estimator):
        fn.argtypes, fn.restype = [C.c_int], None
    return host


def _median_us(e, reps, call):
    out = []
    for r in range(reps + 2):
        e.profile_reset()
        call()
        e.synchronize()
        k, ms = e.profile_get(K_REESTIMATE)
        if r >= 2:
            out.append(ms / max(k, 1))
    return 1e3 * float(np.median(out))


def kernel():
    mh = importlib.import_module("multi-h_amd")
    print(f"== kernel times, median of {REPS} (us): k_label_quantile (1/2); mh_reestimate under \"dlt\" with k_reweight_h at c2 = {THR}^2 "
          f"(fixed) and k_autoscale_reweight_h (auto: 1/2, kappa2 = log2(100), c2 in [DBL_MIN, {C2_MAX:.4f}]) ==", flush=True)
    for n, nh in ((50000, 11), (20000, 540)):
        sc = mh.synth.make_scene(n, 10, seed=1234, with_neighbours=False)
        rng = np.random.default_rng(7)
        lab = np.where(sc.gt_label >= 0, sc.gt_label, rng.integers(-1, nh, size=n)).astype(np.int32)
        H0 = np.tile(sc.H_true, ((nh + 9) // 10, 1))[:nh]
        with mh.Engine(0, 2.6, THR, 0.005, 0.5, 20) as e:
            e.set_correspondences(sc.src, sc.dst)
            e.set_estimator("dlt")
            e.profile_enable(True)
            row = [f"quantile {_median_us(e, REPS, lambda: e.label_residual_quantile(lab, H0, 1, 2)):8.1f}"]

            def reestimate():
                e.set_models(H0)
                e.profile_reset()
                e.reestimate(lab)

            e.set_estimator_reweighting(0, 0.0)
            row.append(f"plain fit {_median_us(e, REPS, reestimate):8.1f}")
            for rounds in (1, 3):
                e.set_estimator_reweighting(rounds, THR * THR)
                fixed = _median_us(e, REPS, reestimate)
                e.set_estimator_reweighting_auto(rounds, *AUTO)
                auto = _median_us(e, REPS, reestimate)
                info = e.reweight_homographies_auto(lab, H0, *AUTO, rounds)[3]
                row.append(f"rounds {rounds}: fixed {fixed:8.1f} auto {auto:8.1f} (+{(auto - fixed) / (rounds + 1):6.1f} per selection; "
                           f"done {info[:, 2].min()}..{info[:, 2].max()})")
        print(f"  {n:6d} points x {nh:3d} labels:  " + "   ".join(row), flush=True)


def rms_to_truth(mh, sc, H, plane):
    g = sc.gt_label == plane
    d = mh.synth.apply_h(H, sc.src[g]) - mh.synth.apply_h(sc.H_true[plane], sc.src[g])
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


def final():
    mh = importlib.import_module("multi-h_amd")
    import reweight_probe as RP
    host = RP._host(mh)
    print("== final refit: Process() (F given, 4 000 hypotheses), then over the run's labels from its models: fixed thr_hom / self-scaled ==",
          flush=True)
    for n, planes in ((20000, 6), (50000, 10)):
        sc = mh.synth.make_scene(n, planes, seed=1234, with_neighbours=False)
        k, labels, H = RP.run_process(host, sc, 99, 4000, 32, True)
        if k < 2:
            sys.exit(f"final {n} / {planes}: Process() returned {k} clusters")
        plane_of = [int(np.bincount(sc.gt_label[(labels == c) & (sc.gt_label >= 0)], minlength=planes).argmax()) for c in range(k)]
        before = [rms_to_truth(mh, sc, H[c], plane_of[c]) for c in range(k)]
        print(f"  {n} / {planes}: {k} clusters; RMS to the true H without a refit: mean {np.mean(before):.4f} px, max {max(before):.4f} px", flush=True)
        with mh.Engine(0, 2.6, THR, 0.005, 0.5, 20) as e:
            e.set_correspondences(sc.src, sc.dst)
            for rounds in (1, 3):
                Hf, gain, info = e.reweight_homographies(labels, H, THR * THR, rounds)
                after = [rms_to_truth(mh, sc, Hf[c], plane_of[c]) for c in range(k)]
                print(f"      fixed {THR:.2f} px, {rounds} round(s): mean {np.mean(after):.4f} px, max {max(after):.4f} px, nearer the truth for "
                      f"{sum(a < b for a, b in zip(after, before))} of {k}; support {info[:, 1].sum()} of {info[:, 0].sum()}", flush=True)
                Ha, gain, scale, info = e.reweight_homographies_auto(labels, H, *AUTO, rounds)
                after = [rms_to_truth(mh, sc, Ha[c], plane_of[c]) for c in range(k)]
                root = np.sqrt(scale[:, 1])
                print(f"      self-scaled, {rounds} round(s):    mean {np.mean(after):.4f} px, max {max(after):.4f} px, nearer the truth for "
                      f"{sum(a < b for a, b in zip(after, before))} of {k}; support {info[:, 1].sum()} of {info[:, 0].sum()}; scale "
                      f"{root.min():.3f}..{root.max():.3f} px, rounds done {info[:, 2].min()}..{info[:, 2].max()}", flush=True)


def barrsmith():
    mh = importlib.import_module("multi-h_amd")
    import barrsmith_agreement as BA
    host = _host(mh)
    print("== barrsmith, the reference's rows, F given, twelve seeds: ARI on the reference's inliers ==", flush=True)
    corr, ref, matched, total = BA.kept_correspondences()
    e = mh.Engine(0, 2.6, THR, 0.005, 0.5, 20)
    e.set_correspondences(corr[:, 0:2], corr[:, 2:4], corr[:, 4:8])
    F, e2, mask, inl = e.estimate_fundamental(1234 ^ 0xf00d, 4000, 2.6)
    e.close()
    for name, fixed, auto in (("--estimator dlt", 0, 0), ("--estimator dlt --estimator-reweight 2", 2, 0),
                              ("--estimator dlt --estimator-reweight-auto 2", 0, 2)):
        rows = []
        try:
            host.mhh_set_estimator(2)
            host.mhh_set_estimator_reweight(fixed)
            host.mhh_set_estimator_reweight_auto(auto)
            for seed in SEEDS:
                k, labels, it, en = BA.run("dlt", corr, F, e2, seed=seed)
                a = BA.agreement(labels, ref) if k > 0 else {"ari_reference_inliers": float("nan")}
                rows.append((int(k), a["ari_reference_inliers"]))
        finally:
            host.mhh_set_estimator(-1)
            host.mhh_set_estimator_reweight(-1)
            host.mhh_set_estimator_reweight_auto(-1)
        aris = sorted(r[1] for r in rows)
        print(f"  {name:44s}: planes {[r[0] for r in rows]}, ARI median {statistics.median(aris):.3f} min {aris[0]:.3f} max {aris[-1]:.3f}", flush=True)


PARTS = {"kernel": kernel, "final": final, "barrsmith": barrsmith}

if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] in PARTS:
        PARTS[sys.argv[1]]()
    else:
        for p in PARTS:
            sys.stdout.flush()
            r = subprocess.run([sys.executable, os.path.abspath(__file__), p], timeout=LIMIT)
            if r.returncode != 0:
                sys.exit(f"label_scale_probe: part {p} ended with status {r.returncode}; nothing more is started")
            print(flush=True)
