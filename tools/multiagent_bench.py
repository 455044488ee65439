#!/usr/bin/env python3
"""Time of one multi-agent round (pcgrl_ma_step: A sub-steps in one launch) against A single-agent turtle pcgrl_step launches
of the same problem, map shape and batch -- the kernel a host-side emulation of a round would run A times (without the A
position uploads it would also need).

    python tools/multiagent_bench.py [--windows 5] [--steps 400] [--warmup 100] [--out profiles/multiagent_bench.json]   # (the default)
    python tools/multiagent_bench.py --only binary:16x16:3:4096:1 --windows 1 --out ''     # one case, for a kernel trace of its own

The two alternate inside one process and the whole cycle repeats `--windows` times, so drift of the machine shows up as spread
inside each column instead of as a difference between columns.  A window is `--steps` rounds (or steps x A launches) on one
stream between two device synchronisations (host clock), after `--warmup` rounds of the same engine; random actions (half
moves, half tiles), auto-reset, engines alive for the whole run.

Algorithmic bytes of a round per env: A observations + A x (reward 4 + done 1 + statistics 4 n_stats) + done_all 1, the state
read and written (tile planes + the 128-byte hot line of the record + positions 8 A + side 16) and the actions 4 A.  The share
of the HBM peak printed with it divides these bytes by the time of the WHOLE call (launch included), not by the kernel's.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from control_pcgrl_amd import MultiAgentVecEnv, VecPcgrlEnv  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--warmup", type=int, default=100)
ap.add_argument("--only", default=None, help="one case: problem:HxW:agents:envs:show, e.g. zelda:16x16:2:4096:0")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                          "multiagent_bench.json"), help="'' writes no file")
args = ap.parse_args()

cases = [(prob, shape, A, n, show) for prob, shape in (("binary", (16, 16)), ("zelda", (16, 16)), ("binary", (40, 16)))
         for A in (2, 3) for n in (4096, 16384) for show in (False, True)]
if args.only:
    prob, shape, A, n, show = args.only.split(":")
    cases = [(prob, tuple(int(v) for v in shape.split("x")), int(A), int(n), bool(int(show)))]
sp = torch.cuda.current_stream().cuda_stream
result = {"method": "host clock around --steps rounds between device synchronisations; a round = one pcgrl_ma_step launch, against "
                    "A pcgrl_step launches of a single-agent turtle engine of the same shape and batch, alternating in one process; "
                    "random actions, auto-reset", "steps": args.steps, "warmup": args.warmup, "windows": args.windows, "rows": []}
for prob, shape, A, n, show in cases:
    g = torch.Generator(device="cuda").manual_seed(1)
    ma = MultiAgentVecEnv(prob, shape, n, A, show_agents=show, seeds=np.arange(n))
    ma.reset()
    pool_ma = torch.randint(0, ma.num_actions, (64, n, A), generator=g, device="cuda", dtype=torch.int32)
    legs = {"round": lambda k: ma.step_raw(pool_ma[k % 64].data_ptr(), sp)}
    one = VecPcgrlEnv(prob, "turtle", shape, n, seeds=np.arange(n))
    one.reset()
    pool_one = torch.randint(0, one.num_actions, (64, A, n), generator=g, device="cuda", dtype=torch.int32)

    def single(k):
        for i in range(A):
            one.step_raw(pool_one[k % 64, i].data_ptr(), sp)
    legs["A_steps"] = single
    for leg in legs.values():
        for k in range(args.warmup):
            leg(k)
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for w in range(args.windows):
        for name, leg in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.steps):
                leg(k + 37 * w)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e6)
    ma.check_errors()
    mbytes = 4 if shape[1] <= 32 else 8
    state = 2 * (4 * shape[0] * mbytes + 128 + 8 * A + 16)
    per_env = A * int(np.prod(ma.obs_shape)) + A * (5 + 4 * ma.n_stats) + 1 + state + 4 * A
    row = {"problem": prob, "shape": list(shape), "agents": A, "envs": n, "show_agents": show, "bytes_per_round": per_env * n}
    for name, t in times.items():
        row[name + "_us"] = {"mean": round(statistics.mean(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
    row["agent_steps_per_s"] = round(n * A / (row["round_us"]["mean"] * 1e-6))
    row["hbm_share_of_peak_whole_call"] = round(per_env * n / (row["round_us"]["mean"] * 1e-6) / HBM_PEAK, 4)
    if "A_steps_us" in row:
        row["round_over_A_steps"] = round(row["round_us"]["mean"] / row["A_steps_us"]["mean"], 3)
    result["rows"].append(row)
    print(json.dumps(row), flush=True)
    ma.close()
    one.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
