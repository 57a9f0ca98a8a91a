"""The move planner of the alpha-expansion (multi-h_amd/csrc/expand_plan.hpp) without a GPU: tests/expand_plan_driver.cpp, which
includes that header alone, plays the device with seeded outcomes and prints every decision; the rules are checked here against
a model written out in full, so the planner's decisions are pinned move by move."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-h_amd", "csrc")
SCHEDULES = [(70, 30, 10, 0), (0,), (100, 0), (50, 50, 0, 20), (15, 5, 5, 5, 5, 0)]    # per cent of a cycle's moves accepted
SEEDS = (1, 2, 3)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")


def _compile(out, extra):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I" + CSRC, os.path.join(ROOT, "tests", "expand_plan_driver.cpp"),
                           "-o", out], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """The driver, and — where the toolchain links the sanitizer runtimes — the same program under ASan + UBSan (run directly)."""
    d = tmp_path_factory.mktemp("plan")
    plain = str(d / "driver")
    b = _compile(plain, [])
    assert b.returncode == 0, b.stderr[-3000:]
    out = [plain]
    san = str(d / "driver_san")
    if _compile(san, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]).returncode == 0:
        out.append(san)
    return out


def _run(exe, L, contexts, min_labels, seed, schedule):
    r = subprocess.run([exe, str(L), str(contexts), str(min_labels), str(seed), *map(str, schedule)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def _check(text, L, contexts, min_labels):
    """Every rule of the planner on one printed run; returns what happened in it."""
    lines = [l.replace("|", " ").split() for l in text.splitlines()]
    assert lines[0] == ["config", str(L), str(contexts), str(min_labels), lines[0][4]]
    cycles = int(lines[0][4])
    seen = dict(batches=0, skips=0, solos=0, halved=0, doubled=0, idempotent_cuts=0, quiet_cycles=0, cut=0)
    t_next, cycle, fresh, known, bsize = 0, 1, True, -1, max(contexts, 1)
    prev, pending, tlast_at_cycle_start = None, None, -1
    for w in lines[1:]:
        kind, v = w[0], list(map(int, w[1:]))
        if kind in ("skip", "solo", "batch"):
            assert pending is None, "a decision while a batch's commit is awaited"
            c, t, alpha = v[0], v[1], v[2]
            assert c == cycle and t == t_next and alpha == t % L and (cycle - 1) * L <= t < cycle * L, w      # in order, each once
            got_fresh, got_known = bool(v[-3 if kind == "batch" else -2]), v[-2 if kind == "batch" else -1]
            assert got_fresh == fresh and (not fresh or got_known == known), (w, fresh, known)
            # the model: today's schedule, written out
            idle = fresh and t >= L and known <= t - L
            batching = contexts > 1 and L >= 2 and (L >= min_labels or cycle >= 2)
            B = min(bsize, L - alpha)
            if fresh and t >= L and not idle and known + L - t < B:
                B = known + L - t                                    # in front of the first move known to be idempotent
                seen["idempotent_cuts"] += kind == "batch"
            want = "skip" if idle else "batch" if batching and B >= 2 else "solo"
            assert kind == want, (w, want, B, bsize)
        if kind == "skip":
            assert fresh and t >= L and known <= t - L                # only on fresh knowledge ...
            assert v[3] == L - alpha                                  # ... and then the whole rest of the cycle
            t_next += v[3]
            seen["skips"] += 1
        elif kind == "solo":
            t_next += 1
            fresh = False
            seen["solos"] += 1
        elif kind == "batch":
            got_B, apply_pending = v[3], v[4]
            assert v[-1] == bsize and 2 <= bsize <= contexts
            assert got_B == B and 2 <= got_B <= contexts and alpha + got_B <= L, w      # never across a cycle's end
            if fresh:
                assert not any(t + k >= L and known <= t + k - L for k in range(got_B)), "a move known to be idempotent inside a batch"
            assert apply_pending == (prev == "solo") == (not fresh), w
            pending = (t, got_B)
            seen["batches"] += 1
        elif kind == "commit":
            j, tlast, new_bsize = v
            t0, B = pending
            assert 1 <= j <= B
            if j < B:
                seen["cut"] += 1
                if 2 * j < B:
                    seen["halved"] += bsize > 2
                    bsize = max(2, bsize // 2)
            elif B == bsize:
                seen["doubled"] += bsize < contexts
                bsize = min(contexts, 2 * bsize)
            assert new_bsize == bsize and 2 <= bsize <= contexts, (w, bsize)
            t_next = t0 + j                                           # the move that failed heads whatever comes next
            fresh, known, pending = True, tlast, None
        elif kind == "end":
            assert pending is None and v[0] == cycle and t_next == cycle * L, (w, t_next)
            seen["quiet_cycles"] += v[1] == tlast_at_cycle_start
            fresh, known, tlast_at_cycle_start = True, v[1], v[1]
            cycle += 1
        else:
            raise AssertionError(w)
        prev = kind
    assert cycle == cycles + 1
    if contexts == 1 or L < 2:
        assert seen["batches"] == 0
    return seen


@pytest.mark.parametrize("min_labels", [0, 16])
@pytest.mark.parametrize("contexts", [1, 2, 3, 16])
@pytest.mark.parametrize("L", [1, 2, 3, 11, 40])
def test_the_planner_follows_its_rules(drivers, L, contexts, min_labels):
    total = {}
    for exe in drivers:
        for schedule in SCHEDULES:
            for seed in SEEDS:
                seen = _check(_run(exe, L, contexts, min_labels, seed, schedule), L, contexts, min_labels)
                for k, n in seen.items():
                    total[k] = total.get(k, 0) + n
    print(L, contexts, min_labels, total, "sanitized run included" if len(drivers) > 1 else "no sanitizer runtime")
    assert total["quiet_cycles"] > 0 and total["skips"] > 0, "cycles in which nothing is accepted must be part of the runs"
    # (two labels batched from the second cycle on never batch: behind a cycle's end the planner knows which of the two moves
    # is idempotent, and a move alone leaves one move in the cycle)
    if contexts > 1 and (L >= 3 or (L == 2 and min_labels == 0)):
        assert total["batches"] > 0 and total["solos"] > 0
    if contexts == 16 and L == 40:                                    # the paths of the batch-size rule all ran
        assert total["halved"] > 0 and total["doubled"] > 0 and total["idempotent_cuts"] > 0 and total["cut"] > 0, total
