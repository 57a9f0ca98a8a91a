"""bench.py's plain run and `--dump-outputs`: the plain line carries the headline alone, and the dumped arrays are what the
timed path computed in its last step — the same in two runs, and the oracle's (20 000 points x 10 000 hypotheses, so that the
whole batch can be checked on the host; R is 1.6 GB, well beyond the caches)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SEED, POINTS, PLANES, MODELS, STEPS, WARMUP = 1234, 20000, 4, 10000, 3, 1


def _plain(dump_dir):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--points", str(POINTS), "--planes", str(PLANES), "--models", str(MODELS), "--seed", str(SEED),
           "--dump-outputs", str(dump_dir)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "bench.py must print exactly one JSON line"
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(dump_dir, f)) for f in sorted(os.listdir(dump_dir))}


def test_plain_run_dumps_its_last_step(mh, oracle, tmp_path):
    O = oracle
    line, got = _plain(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0 and line["value"] > 0
    for k in ("pipelined_form", "strong_split_rehearsal_on_one_gpu", "fused_score", "sustained", "labeling", "full_loop"):
        assert k not in line, f"{k} belongs to --full"
    assert set(got) == {"scores", "best", "models", "samples", "residuals_sample", "residuals_index"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    # the batch of the last timed step: counters (WARMUP + STEPS - 1) * MODELS onwards
    sc = mh.synth.make_scene(POINTS, PLANES, seed=SEED, with_neighbours=False)
    idx = O.sample4(SEED, (WARMUP + STEPS - 1) * MODELS, MODELS, sc.n)
    assert np.array_equal(got["samples"], idx)
    H = got["models"]
    H_ref, wit, _ = O.dlt4(sc.src, sc.dst, idx)
    good = wit > 1e-6
    assert np.max(np.abs(H[good] - H_ref[good])) <= 1e-6
    thr2 = 2.2 * 2.2
    cnt_ref = O.score(sc.src, sc.dst, H, thr2)
    assert np.array_equal(got["scores"], cnt_ref)
    assert got["best"].tolist() == [int(np.argmax(cnt_ref)), int(cnt_ref.max())] == [line["best_model"], line["best_score"]]
    pos = got["residuals_index"].astype(np.int64)
    assert pos.size == 1 << 20 and np.all(np.diff(pos) >= 0) and pos[-1] < MODELS * sc.n
    sel = np.arange(0, pos.size, 4096)                  # 256 of the sampled entries, spread over the whole matrix
    rows = np.unique(pos[sel] // sc.n)
    with np.errstate(all="ignore"):
        R_ref = O.residual_matrix(sc.src, sc.dst, H[rows])
    want = R_ref[np.searchsorted(rows, pos[sel] // sc.n), pos[sel] % sc.n]
    ok = ~np.isnan(want)
    assert ok.sum() > 200
    assert np.array_equal(got["residuals_sample"][sel][ok].view(np.uint64), want[ok].view(np.uint64))

    # the same arguments give the same inputs, hence the same outputs
    _, again = _plain(tmp_path / "b")
    assert set(again) == set(got)
    for k in got:
        assert np.array_equal(got[k], again[k], equal_nan=True), k
