#!/usr/bin/env python3
"""Time per call of LodeRunnerEvaluator.evaluate (control_pcgrl_amd.loderunner) and per launch of the C entry point
pcgrl_loderunner_evaluate on outputs allocated once, on batches of stock-size (8 x 12) Lode Runner maps, next to the plain-Python rules (tests/loderunner_rules.py) on one core of the same host in the same
run.

    python tools/loderunner_bench.py [--levels 4096] [--windows 3] [--window-s 0.5] [--warmup 3] [--out profiles/loderunner_bench.json]

Cases: the three kinds of tests/loderunner_levels.py (random: the problem's _prob with one player; gold: a quarter of the cells
gold; structured: floors, ladders, ropes).  A window is `calls` launches on one stream between two device synchronisations
(host clock), `calls` chosen per case so that a window lasts about --window-s; the cases alternate and the cycle repeats
--windows times, after --warmup launches of each.  Two forms are timed in alternation: `evaluate_us`, a call of evaluate(),
which besides the kernel allocates the output tensors (torch's caching allocator) and enqueues two small torch kernels for the
error word; and `launch_us`, pcgrl_loderunner_evaluate alone on the outputs of an earlier call -- the kernel.  The workspace is
allocated once.  `expanded` counts the cells the rules expand per level over all its searches (the reference's
own work: it skips golds found on earlier paths, the device only those found before a round of 32 golds starts);
`longest_search` is the most cells one search of the batch expands -- a launch lasts at least as long as its slowest level,
whose searches run side by side (both directions of 32 golds per round), so launch time over `longest_search` bounds from
above what one expansion costs the lane that runs it.  Every timed case's outputs are compared with the rules on all its levels."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import loderunner_levels as LL  # noqa: E402
import loderunner_rules as R  # noqa: E402
from control_pcgrl_amd import _lib  # noqa: E402
from control_pcgrl_amd.loderunner import LodeRunnerEvaluator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--levels", type=int, default=4096)
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--window-s", type=float, default=0.5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "loderunner_bench needs the GPU: a host run gives no time"

H, W, CAP = 8, 12, 32
n = args.levels
maps = {k: LL.batch(k, 7000 + i, n, H, W) for i, k in enumerate(LL.KINDS)}
ev = LodeRunnerEvaluator((H, W), "cuda:0", max_levels=n)
dev = {k: torch.as_tensor(v, device="cuda:0") for k, v in maps.items()}
result = {"method": "host clock around `calls` launches between device synchronisations; cases alternate, windows repeated in one "
                    "process; rules on one host core over the same levels in the same run",
          "levels": n, "map_shape": [H, W], "gold_cap": CAP, "warmup": args.warmup, "windows": args.windows,
          "mapping": "one wave per level (blocks: what fits 640 MiB of workspace, 256..4096), one search per lane",
          "cases": {}}


def window(call, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls * 1e6


def launch(k):
    """the C entry point alone, into the tensors the last evaluate() of case k returned"""
    o = last[k]
    _lib.check(ev._L.pcgrl_loderunner_evaluate(
        C.byref(ev._cfg), n, dev[k].data_ptr(), ev._workspace.data_ptr(), ev._workspace_bytes, CAP, o["stats"].data_ptr(),
        o["loss"].data_ptr(), o["play"].data_ptr(), o["gold_state"].data_ptr(), o["gold_dist"].data_ptr(), o["error"].data_ptr(),
        torch.cuda.current_stream().cuda_stream), "pcgrl_loderunner_evaluate")


times, ltimes, calls, last = {k: [] for k in maps}, {k: [] for k in maps}, {}, {}
for k in maps:
    for _ in range(max(1, args.warmup)):
        last[k] = ev.evaluate(dev[k], gold_cap=CAP)
        launch(k)
    once = window(lambda: ev.evaluate(dev[k], gold_cap=CAP), 5)
    calls[k] = int(min(5000, max(5, args.window_s * 1e6 / once)))
    print("warm", k, round(once, 1), "us ->", calls[k], "calls per window", flush=True)
result["workspace_bytes"] = ev._workspace_bytes
for w in range(args.windows):
    for k in maps:
        times[k].append(window(lambda: ev.evaluate(dev[k], gold_cap=CAP), calls[k]))
        ltimes[k].append(window(lambda: launch(k), calls[k]))
        print("window", w, k, "evaluate", round(times[k][-1], 1), "us, launch", round(ltimes[k][-1], 1), "us", flush=True)
ev.check_errors()
last = {k: ev.evaluate(dev[k], gold_cap=CAP) for k in maps}  # (what is compared with the rules below)

for k in maps:
    got = {name: last[k][name].cpu().numpy() for name in ("stats", "play", "gold_state", "gold_dist")}
    t = time.perf_counter()
    answers = [R.get_stats(m) for m in maps[k]]
    rules_s = time.perf_counter() - t
    for i, m in enumerate(maps[k]):
        stats, play, gs, gd = R.outputs(m, CAP) if i < 256 else (None, None, None, None)
        assert got["stats"][i].tolist() == [float(s) for s in answers[i][0]], (k, i)
        if i < 256:
            assert (got["play"][i].tolist(), got["gold_state"][i].tolist(), got["gold_dist"][i].tolist()) == (play, gs, gd), (k, i)
    expanded = np.array([a[1]["expanded"] if a[1] else 0 for a in answers], dtype=np.int64)
    longest = max(a[1]["longest"] if a[1] else 0 for a in answers)
    golds = np.array([a[0][2] for a in answers])
    mean_us = statistics.mean(ltimes[k])
    row = {"calls_per_window": calls[k],
           "evaluate_us": {"mean": round(statistics.mean(times[k]), 1), "min": round(min(times[k]), 1), "max": round(max(times[k]), 1)},
           "launch_us": {"mean": round(mean_us, 1), "min": round(min(ltimes[k]), 1), "max": round(max(ltimes[k]), 1)},
           "levels_per_s": round(n / (statistics.mean(times[k]) * 1e-6), 1),  # of evaluate(), what a caller gets
           "searched_fraction": round(float(np.mean([a[1] is not None for a in answers])), 4),
           "golds": {"mean": round(float(golds.mean()), 2), "max": int(golds.max())},
           "expanded": {"mean": round(float(expanded.mean()), 1), "max": int(expanded.max())},
           "longest_search": int(longest),
           "ns_per_expanded_cell": round(mean_us * 1e3 / max(1.0, float(expanded.sum())), 3),
           "launch_ns_over_longest_search": round(mean_us * 1e3 / max(1, longest), 1),
           "rules": {"levels": n, "seconds": round(rules_s, 3), "levels_per_s": round(n / rules_s, 1)}}
    row["speedup_over_rules_one_core"] = round(row["levels_per_s"] / row["rules"]["levels_per_s"], 1)
    result["cases"][k] = row
    print(k, json.dumps(row), flush=True)
ev.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
