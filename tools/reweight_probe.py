#!/usr/bin/env python3
"""What the reweighted N-point DLT refits (mh_reweight_homographies, csrc/reweight_h.hip; mh_set_estimator_reweighting;
MultiH::SetModelReweight / SetEstimatorReweight) cost and buy, on one MI355X:

  kernel   mh_reestimate's kernel time under "dlt" by the engine's per-kernel events (mh_profile_*), the median of REPS runs
           (default 21), at 50 000 points x 11 labels and 20 000 points x 540 labels: the plain fit (k_dlt_reestimate) beside
           k_reweight_h at 1 and 3 rounds, c2 = thr_hom^2.  Every run starts from the same models.
  final    Process() with the epipolar geometry given on the 20 000 / 6 and 50 000 / 10 synthetic scenes, then the final refit
           MultiH::SetModelReweight(3) runs — mh_reweight_homographies over the run's labels from its models, which
           tests/test_gpu_reweight_h.py holds equal to the hook bit for bit — at the scale thr_hom and at the truncation radius
           thr_hom * 9 / 4: per cluster the RMS distance between H p and H_true p over the points of the plane most of its
           members come from, the mean over the clusters, before and after; the supports and the gains.
  motions  the three-motion scene of DESIGN.md 3.14 (tests/reestimate_dlt_numpy.py::three_motions) at 1 200 and 20 000 points
           through mhh_run_process under SetEpipolarFree(true), without and with SetEstimatorReweight(2) and (3): models, planes
           recovered, ARI, the models' mean RMS distance to the true homographies, LabelingSteps.
  barrsmith  the reference's rows of barrsmith (tools/barrsmith_agreement.py), F given, the twelve seeds of
           profiles/r06_barrsmith_agreement.txt: the default route, SetEstimator(ESTIMATOR_DLT), and that with
           SetEstimatorReweight(2): planes and the ARI on the reference's inliers, median / min / max.

  python tools/reweight_probe.py | grep -v '^\\[Multi-H\\]\\|^Iteration' > profiles/reweight_probe.txt
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
dp = C.POINTER(C.c_double)


def _host(mh):
    host = C.CDLL(os.path.join(os.path.dirname(mh.LIB_PATH), "libmultih_host.so"))
    for fn in (host.mhh_set_model_reweight, host.mhh_set_estimator_reweight, host.mhh_set_estimator, host.mhh_set_epipolar_free):
        fn.argtypes, fn.restype = [C.c_int], None
    return host


def kernel():
    mh = importlib.import_module("multi-h_amd")
    print(f"== mh_reestimate under \"dlt\": kernel time, median of {REPS} (us); rounds 0 = k_dlt_reestimate, else k_reweight_h at c2 = {THR}^2 ==",
          flush=True)
    for n, nh in ((50000, 11), (20000, 540)):
        sc = mh.synth.make_scene(n, 10, seed=1234, with_neighbours=False)
        rng = np.random.default_rng(7)
        lab = np.where(sc.gt_label >= 0, sc.gt_label, rng.integers(-1, nh, size=n)).astype(np.int32)
        H0 = np.tile(sc.H_true, ((nh + 9) // 10, 1))[:nh]
        row = []
        with mh.Engine(0, 2.6, THR, 0.005, 0.5, 20) as e:
            e.set_correspondences(sc.src, sc.dst)
            e.set_estimator("dlt")
            e.profile_enable(True)
            for rounds in (0, 1, 3):
                e.set_estimator_reweighting(rounds, THR * THR)
                out = []
                for r in range(REPS + 2):
                    e.set_models(H0)
                    e.profile_reset()
                    e.reestimate(lab)
                    e.synchronize()
                    k, ms = e.profile_get(K_REESTIMATE)
                    if r >= 2:
                        out.append(ms / max(k, 1))
                info = e.reweight_homographies(lab, H0, THR * THR, max(rounds, 1))[2]
                row.append(f"rounds {rounds} {1e3 * float(np.median(out)):8.1f}" + (f" (done {info[:, 2].min()}..{info[:, 2].max()})" if rounds else ""))
        print(f"  {n:6d} points x {nh:3d} labels:  " + "   ".join(row), flush=True)


def rms_to_truth(mh, sc, H, plane):
    g = sc.gt_label == plane
    d = mh.synth.apply_h(H, sc.src[g]) - mh.synth.apply_h(sc.H_true[plane], sc.src[g])
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


def run_process(host, sc, seed, hypotheses, max_models, given_F):
    labels = np.full(sc.n, -7, dtype=np.int32)
    Hout = np.zeros((256, 9))
    src, dst, aff = (np.ascontiguousarray(a) for a in (sc.src, sc.dst, sc.aff))
    F, e2 = (np.ascontiguousarray(sc.F), np.ascontiguousarray(sc.e2)) if given_F else (None, None)
    k = host.mhh_run_process(src.ctypes.data_as(dp), dst.ctypes.data_as(dp), aff.ctypes.data_as(dp), sc.n,
                             F.ctypes.data_as(dp) if given_F else None, e2.ctypes.data_as(dp) if given_F else None,
                             C.c_double(2.6), C.c_double(THR), C.c_double(0.005), C.c_double(0.5), 20, C.c_ulonglong(seed), hypotheses,
                             max_models, 0, None, 0, labels.ctypes.data_as(C.POINTER(C.c_int)), Hout.ctypes.data_as(dp), 256, None, None,
                             None, 0, 4)
    C.CDLL(None).fflush(None)
    return k, labels, Hout[:max(k, 0)].copy()


def final():
    mh = importlib.import_module("multi-h_amd")
    host = _host(mh)
    print("== final refit: Process() (F given, 4 000 hypotheses), then 3 reweighted rounds over the run's labels from its models ==", flush=True)
    for n, planes in ((20000, 6), (50000, 10)):
        sc = mh.synth.make_scene(n, planes, seed=1234, with_neighbours=False)
        k, labels, H = run_process(host, sc, 99, 4000, 32, True)
        if k < 2:
            sys.exit(f"final {n} / {planes}: Process() returned {k} clusters")
        plane_of = [int(np.bincount(sc.gt_label[(labels == c) & (sc.gt_label >= 0)], minlength=planes).argmax()) for c in range(k)]
        foreign = [float(np.mean(sc.gt_label[labels == c] != plane_of[c])) for c in range(k)]
        before = [rms_to_truth(mh, sc, H[c], plane_of[c]) for c in range(k)]
        print(f"  {n} / {planes}: {k} clusters; members not of the cluster's plane {100 * np.mean(foreign):.1f} % (mean over the clusters, "
              f"max {100 * max(foreign):.1f} %); RMS to the true H without the refit: mean {np.mean(before):.4f} px, max {max(before):.4f} px", flush=True)
        with mh.Engine(0, 2.6, THR, 0.005, 0.5, 20) as e:
            e.set_correspondences(sc.src, sc.dst)
            for name, px in (("thr_hom", THR), ("truncation radius", THR * 9.0 / 4.0)):
                for rounds in (1, 3):
                    Hr, gain, info = e.reweight_homographies(labels, H, px * px, rounds)
                    after = [rms_to_truth(mh, sc, Hr[c], plane_of[c]) for c in range(k)]
                    better = sum(a < b for a, b in zip(after, before))
                    print(f"      scale {px:.2f} px ({name}), {rounds} round(s): mean {np.mean(after):.4f} px, max {max(after):.4f} px, nearer the truth "
                          f"for {better} of {k} clusters; support {info[:, 1].sum()} of {info[:, 0].sum()} members, sum of W {gain[:, 0].sum():.1f} -> "
                          f"{gain[:, 1].sum():.1f}, rounds done {info[:, 2].min()}..{info[:, 2].max()}", flush=True)


def motions():
    mh = importlib.import_module("multi-h_amd")
    import reestimate_dlt_numpy as D
    host = _host(mh)
    print("== three-motion scene through Process() under SetEpipolarFree(true), estimator reweighting off / 2 / 3 rounds at thr_hom ==", flush=True)
    for n in (1200, 20000):
        sc = D.three_motions(n)
        for rounds in (0, 2, 3):
            try:
                host.mhh_set_epipolar_free(1)
                host.mhh_set_estimator_reweight(rounds)
                k, labels, H = run_process(host, sc, 5, 4000, 16, False)
                steps = host.mhh_get_labeling_steps()
            finally:
                host.mhh_set_epipolar_free(0)
                host.mhh_set_estimator_reweight(-1)
            if k < 0:
                print(f"  {n:6d} points, rounds {rounds}: Process() failed", flush=True)
                continue
            got = mh.synth.agreement(sc.gt_label, labels)
            rms = []
            for c in range(k):
                inl = sc.gt_label[(labels == c) & (sc.gt_label >= 0)]
                if inl.size:
                    rms.append(rms_to_truth(mh, sc, H[c], int(np.bincount(inl, minlength=3).argmax())))
            print(f"  {n:6d} points, rounds {rounds}: {k} models, planes {got['planes_recovered']} of {got['planes']}, ARI {got['ari']:.4f}, "
                  f"mean RMS of a model to its plane's true H {np.mean(rms):.4f} px (max {max(rms):.4f}), LabelingSteps {steps}", flush=True)


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
    for name, est, rounds in (("default route (HAF estimator)", -1, 0), ("--estimator dlt", 2, 0), ("--estimator dlt --estimator-reweight 2", 2, 2)):
        rows = []
        try:
            host.mhh_set_estimator(est)
            host.mhh_set_estimator_reweight(rounds)
            for seed in SEEDS:
                k, labels, it, en = BA.run("dlt", corr, F, e2, seed=seed)
                a = BA.agreement(labels, ref) if k > 0 else {"ari_reference_inliers": float("nan")}
                rows.append((int(k), a["ari_reference_inliers"]))
        finally:
            host.mhh_set_estimator(-1)
            host.mhh_set_estimator_reweight(-1)
        aris = sorted(r[1] for r in rows)
        print(f"  {name:40s}: planes {[r[0] for r in rows]}, ARI median {statistics.median(aris):.3f} min {aris[0]:.3f} max {aris[-1]:.3f}", flush=True)


PARTS = {"kernel": kernel, "final": final, "motions": motions, "barrsmith": barrsmith}

if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] in PARTS:
        PARTS[sys.argv[1]]()
    else:
        for p in PARTS:
            sys.stdout.flush()
            r = subprocess.run([sys.executable, os.path.abspath(__file__), p], timeout=LIMIT)
            if r.returncode != 0:
                sys.exit(f"reweight_probe: part {p} ended with status {r.returncode}; nothing more is started")
            print(flush=True)
