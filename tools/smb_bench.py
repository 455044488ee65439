#!/usr/bin/env python3
"""Time per launch of pcgrl_smb_evaluate (control_pcgrl_amd.smb.SmbEvaluator) on batches of stock-size (16 x 116) Mario maps,
next to the plain-Python rules (tests/smb_rules.py, CPython's heapq) on one core of the same host.

    python tools/smb_bench.py [--levels 4096] [--windows 3] [--calls 2] [--warmup 1] [--out profiles/smb_bench.json]

Cases: structured levels (floor, gaps, tubes, platforms, enemies: tests/smb_levels.py), that generator's random levels (mostly
empty, random tile probabilities) and uniform levels (every tile with probability 1/7: the player is walled in and the search
ends early).  A window is `--calls` launches on one stream between two device synchronisations (host clock), after `--warmup`
launches; the cases alternate and the cycle repeats `--windows` times.  Outputs are allocated once per launch by evaluate()
(torch's caching allocator); the workspace once.  `iterations` are the search iterations of both passes per level, from the
launch's own `play` output; `ns_per_iteration` is the launch time over the iterations of the whole batch (throughput, every
level of the batch in flight at once), `ns_per_iteration_longest` the launch time over the longest level's iterations (an
upper bound on what one iteration costs the single lane that runs it).  The results of the timed launches are checked against
the rules on the levels the rules were timed on."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import smb_levels as SL  # noqa: E402
import smb_rules as R  # noqa: E402
from control_pcgrl_amd.smb import SmbEvaluator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--levels", type=int, default=4096)
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--calls", type=int, default=2)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rules-levels", type=int, default=16)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "smb_bench needs the GPU: a host run gives no time"

H, W, POWER = 16, 116, 10000
n = args.levels
t0 = time.perf_counter()
maps = {
    "structured": np.stack([SL.make("structured", 5000 + i, H, W) for i in range(n)]),
    "random": np.stack([SL.make("random", 5000 + i, H, W) for i in range(n)]),
    "uniform": np.random.default_rng(7).integers(0, 7, size=(n, H, W), dtype=np.uint8),
}
print(f"levels made in {time.perf_counter() - t0:.1f} s", flush=True)
ev = SmbEvaluator((H, W), "cuda:0", solver_power=POWER, max_levels=n)
dev = {k: torch.as_tensor(v, device="cuda:0") for k, v in maps.items()}
result = {"method": "host clock around --calls launches between device synchronisations; cases alternate, windows repeated in one "
                    "process; rules on one host core over --rules-levels levels per case",
          "levels": n, "map_shape": [H, W], "solver_power": POWER, "calls": args.calls, "warmup": args.warmup,
          "windows": args.windows, "workspace_bytes": ev._workspace_bytes, "mapping": "one wave per level, search on lane 0",
          "cases": {}}


def window(call, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls * 1e6


times = {k: [] for k in maps}
last = {}
for k in maps:
    for _ in range(max(1, args.warmup)):
        last[k] = ev.evaluate(dev[k])
    torch.cuda.synchronize()
    print("warm", k, flush=True)
for w in range(args.windows):
    for k in maps:
        times[k].append(window(lambda: ev.evaluate(dev[k]), args.calls))
        print("window", w, k, round(times[k][-1], 1), "us", flush=True)
ev.check_errors()

for k in maps:
    play = last[k]["play"].cpu().numpy()
    stats = last[k]["stats"].cpu().numpy()
    iters = (play[:, 4] + play[:, 5]).astype(np.int64)
    m = min(args.rules_levels, n)
    t = time.perf_counter()
    answers = [R.get_stats(maps[k][i], POWER) for i in range(m)]
    rules_s = time.perf_counter() - t
    assert all(answers[i][0] == stats[i].tolist() for i in range(m)), k
    assert all(answers[i][1]["it1"] + answers[i][1]["it2"] == iters[i] for i in range(m)), k
    mean_us = statistics.mean(times[k])
    row = {"launch_us": {"mean": round(mean_us, 1), "min": round(min(times[k]), 1), "max": round(max(times[k]), 1)},
           "levels_per_s": round(n / (mean_us * 1e-6), 1),
           "iterations": {"mean": round(float(iters.mean()), 1), "max": int(iters.max())},
           "won_fraction": round(float(play[:, 0].mean()), 4),
           "ns_per_iteration": round(mean_us * 1e3 / float(iters.sum()), 3),
           "ns_per_iteration_longest": round(mean_us * 1e3 / float(iters.max()), 1),
           "rules": {"levels": m, "levels_per_s": round(m / rules_s, 2),
                     "ns_per_iteration": round(rules_s * 1e9 / float(iters[:m].sum()), 1)}}
    row["speedup_over_rules_one_core"] = round(row["levels_per_s"] / row["rules"]["levels_per_s"], 1)
    result["cases"][k] = row
    print(k, json.dumps(row), flush=True)
ev.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
