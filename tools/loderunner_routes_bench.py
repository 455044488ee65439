#!/usr/bin/env python3
"""What the routes cost (LodeRunnerEvaluator.routes, pcgrl_loderunner_routes), on batches of stock-size
(8 x 12) Lode Runner maps -- the levels of tools/loderunner_bench.py -- in two parts.

    python tools/loderunner_routes_bench.py [--levels 4096] [--windows 3] [--window-s 0.5] [--warmup 3] [--sessions 2]
                                            [--parent-lib control_pcgrl_amd/csrc/libpcgrl_amd_parent.so]
                                            [--out profiles/loderunner_routes_bench.json]

1. The evaluator is not taxed: pcgrl_loderunner_evaluate alone (the C entry point on outputs allocated once), the parent
   commit's build and this build in alternating child processes of one run (--sessions of each; a child loads its library
   through PCGRL_LIB, and the process that starts the children has not touched the device).  --parent-lib is a library built
   from a checkout of the parent commit (its _lib.build(), copied into this package's csrc directory under another name).
   `within_parent_spread`: the mean of this build's windows lies within the minimum and the maximum of the parent's windows.
   Without --parent-lib this part is skipped and the file says so.
2. routes() next to evaluate() on the same maps, in this process: a call of each (outputs allocated by the call) and the two C
   entry points alone on outputs allocated once, in alternation.  `ratio` is routes over evaluate.

A window is `calls` launches on one stream between two device synchronisations (host clock), `calls` chosen per case so that a
window lasts about --window-s; the cases and the forms alternate and the cycle repeats --windows times, after --warmup launches
of each.  Every timed case's routes are compared with the rules' play(m, record=...) on all its levels."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

ap = argparse.ArgumentParser()
ap.add_argument("--levels", type=int, default=4096)
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--window-s", type=float, default=0.5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sessions", type=int, default=2)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--child-evaluate", action="store_true", help="(internal) part 1 in this process, one JSON line")
args = ap.parse_args()

H, W, CAP = 8, 12, 32
n = args.levels


def spread(v):
    return {"mean": round(statistics.mean(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


# ---- part 1, the parent: start the children before this process touches the device
ab = None
if args.parent_lib and not args.child_evaluate:
    parent = os.path.realpath(args.parent_lib)
    assert os.path.exists(parent), parent
    ab = {"parent": {}, "this": {}}
    for s in range(args.sessions):
        for build in ("parent", "this"):
            env = dict(os.environ)
            env.pop("PCGRL_LIB", None)
            if build == "parent":
                env["PCGRL_LIB"] = parent
            cmd = [sys.executable, os.path.abspath(__file__), "--child-evaluate", "--levels", str(n), "--windows", str(args.windows),
                   "--window-s", str(args.window_s), "--warmup", str(args.warmup)]
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True).stdout
            got = json.loads(out.strip().splitlines()[-1])
            for k, v in got.items():
                ab[build].setdefault(k, []).extend(v)
            print("session", s, build, {k: [round(x, 1) for x in v] for k, v in got.items()}, flush=True)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import loderunner_levels as LL  # noqa: E402
import loderunner_routes_expect as X  # noqa: E402
from control_pcgrl_amd import _lib  # noqa: E402
from control_pcgrl_amd.loderunner import LodeRunnerEvaluator  # noqa: E402

assert torch.cuda.is_available(), "loderunner_routes_bench needs the GPU: a host run gives no time"
maps = {k: LL.batch(k, 7000 + i, n, H, W) for i, k in enumerate(LL.KINDS)}  # tools/loderunner_bench.py's levels
ev = LodeRunnerEvaluator((H, W), "cuda:0", max_levels=n)
dev = {k: torch.as_tensor(v, device="cuda:0") for k, v in maps.items()}
ROUTE_CAP = 8 * H * W


def window(call, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls * 1e6


def launch_evaluate(k):
    o = last_e[k]
    _lib.check(ev._L.pcgrl_loderunner_evaluate(
        C.byref(ev._cfg), n, dev[k].data_ptr(), ev._workspace.data_ptr(), ev._workspace_bytes, CAP, o["stats"].data_ptr(),
        o["loss"].data_ptr(), o["play"].data_ptr(), o["gold_state"].data_ptr(), o["gold_dist"].data_ptr(), o["error"].data_ptr(),
        torch.cuda.current_stream().cuda_stream), "pcgrl_loderunner_evaluate")


def launch_routes(k):
    o = last_r[k]
    _lib.check(ev._L.pcgrl_loderunner_routes(
        C.byref(ev._cfg), n, dev[k].data_ptr(), ev._workspace.data_ptr(), ev._workspace_bytes, CAP, ROUTE_CAP,
        o["stats"].data_ptr(), o["loss"].data_ptr(), o["play"].data_ptr(), o["gold_state"].data_ptr(), o["gold_dist"].data_ptr(),
        o["gold_off"].data_ptr(), o["gold_back"].data_ptr(), o["coords"].data_ptr(), o["moves"].data_ptr(),
        o["tour_len"].data_ptr(), o["error"].data_ptr(), torch.cuda.current_stream().cuda_stream), "pcgrl_loderunner_routes")


last_e, last_r, calls = {}, {}, {}
for k in maps:
    for _ in range(max(1, args.warmup)):
        last_e[k] = ev.evaluate(dev[k], gold_cap=CAP)
        launch_evaluate(k)
    once = window(lambda: launch_evaluate(k), 5)
    calls[k] = int(min(5000, max(5, args.window_s * 1e6 / once)))

if args.child_evaluate:
    t = {k: [] for k in maps}
    for w in range(args.windows):
        for k in maps:
            t[k].append(window(lambda: launch_evaluate(k), calls[k]))
    print(json.dumps(t))
    sys.exit(0)

forms = {"evaluate_us": lambda k: ev.evaluate(dev[k], gold_cap=CAP), "routes_us": lambda k: ev.routes(dev[k], gold_cap=CAP, moves=True),
         "evaluate_launch_us": launch_evaluate, "routes_launch_us": launch_routes}
for k in maps:
    for _ in range(max(1, args.warmup)):
        last_r[k] = ev.routes(dev[k], gold_cap=CAP, moves=True)
        launch_routes(k)
times = {k: {f: [] for f in forms} for k in maps}
for w in range(args.windows):
    for k in maps:
        for f, call in forms.items():
            times[k][f].append(window(lambda: call(k), calls[k]))
        print("window", w, k, {f: round(v[-1], 1) for f, v in times[k].items()}, flush=True)
ev.check_errors()

result = {"method": "host clock around `calls` launches between device synchronisations; cases and forms alternate, windows repeated "
                    "in one process; the parent's build and this build in alternating child processes of the same run",
          "levels": n, "map_shape": [H, W], "gold_cap": CAP, "route_cap": ROUTE_CAP, "moves": True, "warmup": args.warmup,
          "windows": args.windows, "sessions": args.sessions if ab else 0, "cases": {},
          "not_measured": ["kernel durations under a trace (host clock only)", "shapes other than 8 x 12", "route_cap = 0 (lengths only)",
                           "split_routes (host side)"] + ([] if ab else ["the parent's build next to this one (no --parent-lib)"])}
for k in maps:
    got = {name: v.cpu().numpy() for name, v in ev.routes(dev[k], gold_cap=CAP, moves=True).items()}
    t0 = time.perf_counter()
    pairs = [X.pairs_of_rules(m) for m in maps[k]]
    rules_s = time.perf_counter() - t0
    want = X.expect(pairs, CAP, ROUTE_CAP)
    for name, v in want.items():
        assert np.array_equal(got[name], v), (k, name)
    tours = np.array([sum(len(a[0]) + len(b[0]) for _, a, b in p) for p in pairs])
    longest = max((max(len(a[0]), len(b[0])) for p in pairs for _, a, b in p), default=0)
    row = {"calls_per_window": calls[k]}
    for f in forms:
        row[f] = spread(times[k][f])
    row["ratio"] = {"call": round(row["routes_us"]["mean"] / row["evaluate_us"]["mean"], 4),
                    "launch": round(row["routes_launch_us"]["mean"] / row["evaluate_launch_us"]["mean"], 4)}
    row["routes"] = {"levels_with_a_route": int((tours > 0).sum()), "counted_golds": int(sum(len(p) for p in pairs)),
                     "tour_cells": {"mean": round(float(tours.mean()), 2), "max": int(tours.max())}, "longest_route": int(longest)}
    row["rules"] = {"levels": n, "seconds": round(rules_s, 3), "compared": "coords, moves, tour_len, gold_off, gold_back of every level"}
    if ab:
        p, t = ab["parent"][k], ab["this"][k]
        row["evaluate_alone"] = {"parent_us": spread(p), "this_us": spread(t), "parent_windows": [round(x, 1) for x in p],
                                 "this_windows": [round(x, 1) for x in t],
                                 "within_parent_spread": bool(min(p) <= statistics.mean(t) <= max(p))}
    result["cases"][k] = row
    print(k, json.dumps(row), flush=True)
ev.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
