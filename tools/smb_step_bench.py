#!/usr/bin/env python3
"""Time per launch of SmbVecEnv.step (pcgrl_smb_env_step) on stock-size (16 x 116) Mario envs at solver_power 10000.

    python tools/smb_step_bench.py [--envs 4096] [--steps 200] [--windows 3] [--warmup 5] [--out profiles/smb_step_bench.json]

Cases, each `--steps` launches with random actions after a fresh start (NOT whole episodes: an episode is 5 569 steps):
  narrow_reset, turtle_reset            from reset() -- drawn maps, dense, most searches end early
  narrow_structured, turtle_structured  from reset(init_grids = structured levels of tests/smb_levels.py)
  floor_scans                           narrow on empty maps writing non-solid tiles only: no env ever changes solidity, so a
                                        launch is the scans, the observation and the state -- the floor of a step
  floor_moves                           turtle moving only: no env changes anything (observation and state alone)
A window is `--steps` launches on one stream between two device synchronisations (host clock), after `--warmup` launches; the
cases alternate and the cycle repeats `--windows` times; every window starts from the same fresh start.  Beside them:
  evaluate    SmbEvaluator.evaluate on the maps the case holds after its last window: what a step without the two shortcuts
              would pay in every launch
  rules       tests/smb_env_rules.py on one host core, one env, the same shape and actions: the CPU figure
Iterations per step are the device's own counters (get_state().search_iterations / max_search_iterations).  The cases of one
representation share an env object and max_search_iterations is kept over the object's life, so `iterations_max_in_one_call` of
a case is the most any call spent on one env in that case OR an earlier case of the same representation (the floors' figure
is their predecessors')."""
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

import smb_env_rules as E  # noqa: E402
import smb_levels as SL  # noqa: E402
from control_pcgrl_amd import SmbVecEnv  # noqa: E402
from control_pcgrl_amd.smb import SmbEvaluator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rules-steps", type=int, default=60)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "smb_step_bench needs the GPU: a host run gives no time"

H, W, POWER, DEV = 16, 116, 10000, "cuda:0"
n, T = args.envs, args.steps
rng = np.random.default_rng(11)
structured = torch.as_tensor(np.stack([SL.make("structured", 7000 + i, H, W) for i in range(n)]), device=DEV)
empty = torch.zeros((n, H, W), dtype=torch.uint8, device=DEV)
nonsolid = np.array([0, 2, 5])
CASES = {  # name: (representation, init_grids, actions [T + warmup][n])
    "narrow_reset": ("narrow", None, rng.integers(0, 7, (T + args.warmup, n))),
    "turtle_reset": ("turtle", None, rng.integers(0, 11, (T + args.warmup, n))),
    "narrow_structured": ("narrow", structured, rng.integers(0, 7, (T + args.warmup, n))),
    "turtle_structured": ("turtle", structured, rng.integers(0, 11, (T + args.warmup, n))),
    "floor_scans": ("narrow", empty, nonsolid[rng.integers(0, 3, (T + args.warmup, n))]),
    "floor_moves": ("turtle", empty, rng.integers(0, 4, (T + args.warmup, n))),
}
envs = {rep: SmbVecEnv(rep, (H, W), n, device=DEV, solver_power=POWER, seeds=np.arange(n)) for rep in ("narrow", "turtle")}
ev = SmbEvaluator((H, W), DEV, solver_power=POWER, max_levels=n)
actions = {k: torch.as_tensor(v[2], dtype=torch.int32, device=DEV) for k, v in CASES.items()}
result = {"method": "host clock around --steps step launches between device synchronisations, after --warmup launches from a "
                    "fresh start (re-seeded reset, or reset(init_grids)); cases alternate, windows repeated in one process",
          "envs": n, "map_shape": [H, W], "solver_power": POWER, "steps": T, "warmup": args.warmup, "windows": args.windows,
          "obs_bytes_per_launch": n * 2 * H * 2 * W * 8, "cases": {}}
times = {k: [] for k in CASES}
counters = {}


def fresh(k):
    rep, grids, _ = CASES[k]
    env = envs[rep]
    env.seed(np.arange(n))
    env.reset(init_grids=grids)
    return env


for w in range(args.windows):
    for k in CASES:
        env, a = fresh(k), actions[k]
        for t in range(args.warmup):
            env.step(a[t])
        s0 = env.get_state()
        it0, se0 = s0.search_iterations.clone(), s0.searches.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(args.warmup, args.warmup + T):
            env.step(a[t])
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) / T * 1e6)
        s1 = env.get_state()
        counters[k] = {"iterations_per_env_step_mean": round(float((s1.search_iterations - it0).sum()) / (n * T), 2),
                       "iterations_max_in_one_call": int(s1.max_search_iterations.max()),
                       "searches_per_env_step": round(float((s1.searches - se0).sum()) / (n * T), 4)}
        print("window", w, k, round(times[k][-1], 1), "us", counters[k], flush=True)
        if w == args.windows - 1:  # the same maps through the evaluator: a step without the shortcuts
            grids = s1.grids.clone()
            ev.evaluate(grids, playthrough=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.evaluate(grids, playthrough=False)
            torch.cuda.synchronize()
            counters[k]["evaluate_same_maps_us"] = round((time.perf_counter() - t0) * 1e6, 1)
        env.check_errors()

for k, (rep, grids, acts) in CASES.items():
    mean_us = statistics.mean(times[k])
    row = {"launch_us": {"mean": round(mean_us, 1), "min": round(min(times[k]), 1), "max": round(max(times[k]), 1)},
           "env_steps_per_s": round(n / (mean_us * 1e-6), 1)}
    row.update(counters[k])
    m = min(args.rules_steps, T)  # the rules on one host core: env 0 of the case, the same actions
    rules = E.SmbEnvRules(rep, (H, W), seed=0, solver_power=POWER)
    rules.reset(None if grids is None else grids[0].cpu().numpy())
    t0 = time.perf_counter()
    for t in range(m):
        rules.step(int(acts[t, 0]))
    row["rules_one_core"] = {"steps": m, "env_steps_per_s": round(m / (time.perf_counter() - t0), 2)}
    result["cases"][k] = row
    print(k, json.dumps(row), flush=True)
for env in envs.values():
    env.close()
ev.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
