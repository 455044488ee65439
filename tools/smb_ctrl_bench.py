#!/usr/bin/env python3
"""What controllable generation costs a Super Mario Bros step launch, on stock-size (16 x 116) envs at
solver_power 10000.  Three commands:

    python tools/smb_ctrl_bench.py step --out run.json    (a) four cases of tools/smb_step_bench.py -- floor_scans, floor_moves,
        narrow_reset, turtle_reset -- with the library PCGRL_LIB names (or the tree's): run it parent, head, parent, head, each
        in a process of its own, to see whether NON-controllable stepping has become slower
    python tools/smb_ctrl_bench.py ctrl --out ctrl.json   (b) the head alone: the same starts and actions without controls and
        with K = 2 and K = 9 controls, resampling off and on, float64 rewards everywhere
    python tools/smb_ctrl_bench.py merge --parent p1.json p2.json --head h1.json h2.json --ctrl ctrl.json --out profiles/smb_ctrl_bench.json

A window is `--steps` launches on one stream between two device synchronisations (host clock), after `--warmup` launches from a
fresh start (re-seeded reset, or reset(init_grids)); the cases or variants alternate and the cycle repeats `--windows` times.
The condition `merge` evaluates on the floor cases: the head's median is at most the parent's median plus the parent's own
spread (max - min over its windows and both its runs)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("command", choices=["step", "ctrl", "merge"])
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--parent", nargs="*", default=[])
ap.add_argument("--head", nargs="*", default=[])
ap.add_argument("--ctrl", default=None)
args = ap.parse_args()
H, W, POWER, DEV = 16, 116, 10000, "cuda:0"
FLOORS = ("floor_scans", "floor_moves")
ALL9 = ["dist-floor", "disjoint-tubes", "enemies", "empty", "noise", "jumps", "jumps-dist", "dist-win", "sol-length"]


def dump(result):
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if args.command == "merge":
    def runs(paths):
        return [json.load(open(p)) for p in paths]

    parent, head = runs(args.parent), runs(args.head)
    out = {"what": "tools/smb_ctrl_bench.py: (a) non-controllable stepping, parent against head, processes alternating in one "
                   "visit; (b) controllable against non-controllable in the head",
           "a_step": {}, "b_ctrl": json.load(open(args.ctrl)) if args.ctrl else None}
    for k in parent[0]["cases"]:
        p = [t for r in parent for t in r["cases"][k]["windows_us"]]
        h = [t for r in head for t in r["cases"][k]["windows_us"]]
        row = {"parent_windows_us": p, "head_windows_us": h, "parent_median_us": round(statistics.median(p), 2),
               "head_median_us": round(statistics.median(h), 2), "parent_spread_us": round(max(p) - min(p), 2)}
        if k in FLOORS:
            row["condition_head_median_le_parent_median_plus_spread"] = bool(
                statistics.median(h) <= statistics.median(p) + (max(p) - min(p)))
        out["a_step"][k] = row
    out["libraries"] = {"parent": [r["library"] for r in parent], "head": [r["library"] for r in head]}
    dump(out)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from control_pcgrl_amd import SmbVecEnv  # noqa: E402

assert torch.cuda.is_available(), "smb_ctrl_bench needs the GPU: a host run gives no time"
n, T = args.envs, args.steps
rng = np.random.default_rng(11)
empty = torch.zeros((n, H, W), dtype=torch.uint8, device=DEV)
nonsolid = np.array([0, 2, 5])
CASES = {  # name: (representation, init_grids, actions [T + warmup][n]) -- as tools/smb_step_bench.py draws them
    "narrow_reset": ("narrow", None, rng.integers(0, 7, (T + args.warmup, n))),
    "turtle_reset": ("turtle", None, rng.integers(0, 11, (T + args.warmup, n))),
    "floor_scans": ("narrow", empty, nonsolid[rng.integers(0, 3, (T + args.warmup, n))]),
    "floor_moves": ("turtle", empty, rng.integers(0, 4, (T + args.warmup, n))),
}
actions = {k: torch.as_tensor(v[2], dtype=torch.int32, device=DEV) for k, v in CASES.items()}


def window(env, k):
    env.seed(np.arange(n))
    env.reset(init_grids=CASES[k][1])
    a = actions[k]
    for t in range(args.warmup):
        env.step(a[t])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.warmup, args.warmup + T):
        env.step(a[t])
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / T * 1e6
    env.check_errors()
    return round(us, 2)


base = {"envs": n, "map_shape": [H, W], "solver_power": POWER, "steps": T, "warmup": args.warmup, "windows": args.windows,
        "library": os.environ.get("PCGRL_LIB") or "the tree's"}
if args.command == "step":
    envs = {rep: SmbVecEnv(rep, (H, W), n, device=DEV, solver_power=POWER, seeds=np.arange(n)) for rep in ("narrow", "turtle")}
    times = {k: [] for k in CASES}
    for w in range(args.windows):
        for k in CASES:
            times[k].append(window(envs[CASES[k][0]], k))
            print("window", w, k, times[k][-1], "us", flush=True)
    base["cases"] = {k: {"windows_us": v, "median_us": round(statistics.median(v), 2)} for k, v in times.items()}
    dump(base)
else:
    VARIANTS = {"plain": (None, False), "k2": (["jumps", "sol-length"], False), "k2_resampling": (["jumps", "sol-length"], True),
                "k9": (ALL9, False), "k9_resampling": (ALL9, True)}
    envs = {}
    for v, (controls, resample) in VARIANTS.items():
        for rep in ("narrow", "turtle"):
            e = SmbVecEnv(rep, (H, W), n, device=DEV, solver_power=POWER, seeds=np.arange(n), reward_dtype=torch.float64,
                          controls=controls)
            if controls:
                e.sample_uniform_targets(generator=torch.Generator(device=DEV).manual_seed(1))
                e.set_target_resampling(resample, seed=5)
            envs[(v, rep)] = e
    times = {k: {v: [] for v in VARIANTS} for k in CASES}
    for w in range(args.windows):
        for k in CASES:
            for v in VARIANTS:
                times[k][v].append(window(envs[(v, CASES[k][0])], k))
                print("window", w, k, v, times[k][v][-1], "us", flush=True)
    base["note"] = ("every window starts with a reset, which takes the queued or resampled targets; no episode ends inside a "
                    "window (an episode is 5 569 steps), so the windows time the record's load and the control observation, not "
                    "the take")
    base["cases"] = {k: {v: {"windows_us": t, "median_us": round(statistics.median(t), 2)} for v, t in tv.items()}
                     for k, tv in times.items()}
    dump(base)
