#!/usr/bin/env python3
"""Env-steps per second of SmbVecEnv.rollout (pcgrl_smb_env_rollout: K steps in one launch) against K SmbVecEnv.step launches
timed in the same run, on stock-size (16 x 116) Mario envs at solver_power 10000.

    python tools/smb_rollout_bench.py [--envs 4096] [--ks 1,4,16,64,256] [--windows 3] [--warmup 5] [--min-steps 64]
                                      [--out profiles/smb_rollout_bench.json]

The four searching cases of tools/smb_step_bench.py -- narrow and turtle, from reset() and from structured levels -- with the
same fresh starts and random actions.  For every case and K a window covers S = max(K, --min-steps) steps of every env after
`--warmup` step() launches from the fresh start, between two device synchronisations (host clock):
  rollout  S / K launches of rollout(actions[t : t + K], want_obs="last"): the observation is written once per launch
  step     S launches of step(actions[t]) on the same start and the same actions: the parent's path, which the rollout does
           not touch -- the yardstick.  K = 1 against it is the fixed cost of the loop form.
  ready    for context, step_ready at the budget profiles/smb_ready_bench.json names best for the case, until the batch has
           emitted envs * max(--ks) transitions (as tools/smb_ready_bench.py counts them); once per case and cycle.
The cases, the Ks and the three paths alternate and the cycle repeats `--windows` times.  After every timed pair the two envs'
exported states are compared: the rollout must leave what the steps leave.

The structural check, outside the timed windows: for every case and K up to `--structure-launches` single launches from the
same start, each between two synchronisations with get_state().search_iterations read before and after.  A launch should last
about (the largest per-env sum of search iterations in it) x (time per iteration, 2.7-2.8 us in DESIGN.md sections 17 and
18); `us_per_iteration_of_the_slowest_env` is launch time over that largest sum."""
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
from control_pcgrl_amd import SmbReadyVecEnv, SmbVecEnv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--ks", default="1,4,16,64,256")
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--min-steps", type=int, default=64)
ap.add_argument("--chunk", type=int, default=25)
ap.add_argument("--structure-launches", type=int, default=4)
ap.add_argument("--window-seconds", type=float, default=60.0, help="a ready window that lasts longer is given up (the run fails)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "smb_rollout_bench needs the GPU: a host run gives no time"

H, W, POWER, DEV = 16, 116, 10000, "cuda:0"
n = args.envs
KS = [int(k) for k in args.ks.split(",")]
T = max(max(KS), args.min_steps)  # the most steps a window covers
US_PER_ITERATION = (2.7, 2.8)  # DESIGN.md sections 17 and 18
rng = np.random.default_rng(11)  # the cases, maps and actions of tools/smb_step_bench.py
structured = torch.as_tensor(np.stack([SL.make("structured", 7000 + i, H, W) for i in range(n)]), device=DEV)
CASES = {  # name: (representation, init_grids, actions [warmup + T][n])
    "narrow_reset": ("narrow", None, rng.integers(0, 7, (T + args.warmup, n))),
    "turtle_reset": ("turtle", None, rng.integers(0, 11, (T + args.warmup, n))),
    "narrow_structured": ("narrow", structured, rng.integers(0, 7, (T + args.warmup, n))),
    "turtle_structured": ("turtle", structured, rng.integers(0, 11, (T + args.warmup, n))),
}
actions = {k: torch.as_tensor(v[2], dtype=torch.int32, device=DEV) for k, v in CASES.items()}
BEST_BUDGET = {"narrow_reset": 64, "turtle_reset": 32, "narrow_structured": 128, "turtle_structured": 128}
budget_source = "defaults of this tool"
try:
    with open(os.path.join(ROOT, "profiles", "smb_ready_bench.json")) as f:
        BEST_BUDGET.update({k: int(v["best_budget"]) for k, v in json.load(f)["cases"].items() if k in CASES})
    budget_source = "profiles/smb_ready_bench.json"
except (OSError, KeyError, ValueError):
    pass


def make(cls, **kw):
    return {rep: cls(rep, (H, W), n, device=DEV, solver_power=POWER, seeds=np.arange(n), **kw) for rep in ("narrow", "turtle")}


roll_envs, step_envs, ready_envs = make(SmbVecEnv), make(SmbVecEnv), make(SmbReadyVecEnv, solver_budget=4 * POWER)


def fresh(envs, k):
    """the case's start: re-seeded, reset, and --warmup step launches (a ready env takes them under a budget no search exceeds,
    which equals synchronous stepping)"""
    rep, grids, _ = CASES[k]
    env, a = envs[rep], actions[k]
    if envs is ready_envs:
        env.set_solver_budget(4 * POWER)
    env.seed(np.arange(n))
    env.reset(init_grids=grids)
    for t in range(args.warmup):
        if envs is ready_envs:
            env.step_ready(a[t])
        else:
            env.step(a[t])
    return env, a


def rollout_window(k, K, S):
    env, a = fresh(roll_envs, k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.warmup, args.warmup + S, K):
        env.rollout(a[t:t + K], want_obs="last")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env.check_errors()
    return {"launch_us": dt / (S // K) * 1e6, "env_steps_per_s": n * S / dt}, env


def step_window(k, S):
    env, a = fresh(step_envs, k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.warmup, args.warmup + S):
        env.step(a[t])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env.check_errors()
    return {"launch_us": dt / S * 1e6, "env_steps_per_s": n * S / dt}, env


def ready_window(k, S):
    env, a = fresh(ready_envs, k)
    assert int(env.env_busy().sum()) == 0
    env.set_solver_budget(BEST_BUDGET[k])
    rows = a.shape[0]
    start = int(env.get_state().iteration.sum())  # (synchronises)
    launches, emitted, t = 0, 0, args.warmup
    t0 = time.perf_counter()
    while emitted < n * S:
        for _ in range(args.chunk):
            env.step_ready(a[t % rows])
            t += 1
        launches += args.chunk
        emitted = int(env.get_state().iteration.sum()) - start
        dt = time.perf_counter() - t0
        if dt > args.window_seconds:
            raise SystemExit(f"{k} at budget {BEST_BUDGET[k]}: {emitted} of {n * S} transitions after {dt:.1f} s -- given up")
    env.check_errors()
    return {"launch_us": dt / launches * 1e6, "env_steps_per_s": emitted / dt}


def structure(k, K):
    """single launches from the case's start, each with the per-env search iterations it spent"""
    env, a = fresh(roll_envs, k)
    rows = []
    launches = min(args.structure_launches, max(1, args.min_steps // K))
    for j in range(launches):
        t = args.warmup + j * K
        if t + K > a.shape[0]:
            break
        before = env.get_state().search_iterations.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.rollout(a[t:t + K], want_obs="last")
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) * 1e6
        spent = env.get_state().search_iterations - before
        most, mean = int(spent.max()), float(spent.double().mean())
        rows.append({"launch_us": round(us, 1), "iterations_of_the_slowest_env": most, "iterations_per_env_mean": round(mean, 1),
                     "predicted_us": [round(most * u, 1) for u in US_PER_ITERATION],
                     "us_per_iteration_of_the_slowest_env": round(us / most, 3) if most else None})
    return rows


def spread(rows, key):
    v = [r[key] for r in rows]
    return {"mean": round(statistics.mean(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


roll_w = {k: {K: [] for K in KS} for k in CASES}
step_w = {k: {K: [] for K in KS} for k in CASES}
ready_w = {k: [] for k in CASES}
for w in range(args.windows):
    for k in CASES:
        for K in KS:
            S = max(K, args.min_steps) // K * K
            r, env_r = rollout_window(k, K, S)
            s, env_s = step_window(k, S)
            assert torch.equal(env_r.export_state(), env_s.export_state()), (k, K, "the rollout left another state than the steps")
            roll_w[k][K].append(r)
            step_w[k][K].append(s)
            print("window", w, k, "K", K, "steps", S, "rollout", {x: round(v, 1) for x, v in r.items()},
                  "step", {x: round(v, 1) for x, v in s.items()}, flush=True)
        ready_w[k].append(ready_window(k, T))
        print("window", w, k, "ready at budget", BEST_BUDGET[k], {x: round(v, 1) for x, v in ready_w[k][-1].items()}, flush=True)

result = {"method": "host clock between device synchronisations; per case and K a window covers S = max(K, min_steps) steps of "
                    "every env after --warmup step launches from a fresh start: S / K rollout launches (want_obs=last) against S "
                    "step launches on the same start and actions; ready: step_ready at the named budget until envs * max(K) "
                    "transitions were emitted; cases, Ks and paths alternate, windows repeated in one process; the exported "
                    "states of the rollout env and the step env are compared after every pair",
          "envs": n, "map_shape": [H, W], "solver_power": POWER, "ks": KS, "warmup": args.warmup, "windows": args.windows,
          "min_steps": args.min_steps, "ready_budget_source": budget_source, "us_per_iteration_expected": list(US_PER_ITERATION),
          "cases": {}}
for k in CASES:
    row = {"ready": {"budget": BEST_BUDGET[k], "launch_us": spread(ready_w[k], "launch_us"),
                     "env_steps_per_s": spread(ready_w[k], "env_steps_per_s")}, "k": {}}
    for K in KS:
        r, s = roll_w[k][K], step_w[k][K]
        ratios = [a["env_steps_per_s"] / b["env_steps_per_s"] for a, b in zip(r, s)]  # window by window: the pair ran back to back
        rr, ss = spread(r, "env_steps_per_s"), spread(s, "env_steps_per_s")
        row["k"][str(K)] = {
            "steps_per_window": max(K, args.min_steps) // K * K,
            "rollout": {"launch_us": spread(r, "launch_us"), "env_steps_per_s": rr},
            "step": {"launch_us": spread(s, "launch_us"), "env_steps_per_s": ss},
            "rollout_over_step": {"mean": round(statistics.mean(ratios), 3), "min": round(min(ratios), 3), "max": round(max(ratios), 3)},
            "rollout_over_ready": round(rr["mean"] / row["ready"]["env_steps_per_s"]["mean"], 3),
            "differs_from_step_by_more_than_the_spread": bool(rr["min"] > ss["max"] or rr["max"] < ss["min"]),
            "structure": structure(k, K)}
    result["cases"][k] = row
    print(k, json.dumps(row), flush=True)
for env in list(roll_envs.values()) + list(step_envs.values()) + list(ready_envs.values()):
    env.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
