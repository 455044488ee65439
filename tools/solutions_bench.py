#!/usr/bin/env python3
"""Time per call of pcgrl_solutions_for_grids next to pcgrl_stats_for_grids_h on the same sokoban levels: the solved levels of
the committed fixtures (tests/golden/solutions/rooms_16x16.npz and the 16 x 16 solver fixtures) and a batch of random 16 x 16
maps, of which almost none meets the solver's precondition.

    python tools/solutions_bench.py [--windows 5] [--calls 20] [--warmup 5] [--out profiles/solutions_bench.json]

The method of tools/paths_bench.py: a window is `--calls` calls on one stream between two device synchronisations (host
clock), after `--warmup` calls; the two entry points alternate inside one process and the cycle repeats `--windows` times,
so drift of the machine shows up as spread inside a column instead of as a difference between columns.  Both write into
buffers allocated once.  There is no bar: this is a query, and stats_for_grids runs a level's four stages side by side on helper
waves while the solution kernel runs them one after the other on one wave.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from control_pcgrl_amd import VecPcgrlEnv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--random", type=int, default=4096)
ap.add_argument("--out", default=None)
args = ap.parse_args()

GOLDEN = os.path.join(ROOT, "tests", "golden")
solved = []
z = np.load(os.path.join(GOLDEN, "solutions", "rooms_16x16.npz"))
solved += list(z["grids"][z["length"] > 0])
for f in ("stats_sokoban.npz", "stats_sokoban_solver.npz"):
    z = np.load(os.path.join(GOLDEN, f))
    solved += list(z["grids"][z["stats"][:, 5] > 0])
rng = np.random.default_rng(1)
sets = {"solved fixture levels": np.array(solved, np.uint8),
        "random maps": rng.integers(0, 5, (args.random, 16, 16)).astype(np.uint8)}

sp = torch.cuda.current_stream().cuda_stream
result = {"method": "host clock around --calls calls between device synchronisations, solutions_for_grids (cap = solver_power, "
                    "dist_win) and stats_for_grids alternating on the same maps, windows repeated in one process",
          "calls": args.calls, "warmup": args.warmup, "windows": args.windows, "us_per_call": {}}
env = VecPcgrlEnv("sokoban", "narrow", (16, 16), 4)
L, h = env._L, env._h
cap = int(L.pcgrl_solution_capacity(h))
for name, grids in sets.items():
    n = len(grids)
    g = torch.as_tensor(grids, device="cuda").contiguous()
    moves = torch.empty((n, cap), dtype=torch.int8, device="cuda")
    length = torch.empty(n, dtype=torch.int32, device="cuda")
    dist_win = torch.empty(n, dtype=torch.int32, device="cuda")
    stats = torch.empty((n, env.n_stats), dtype=torch.int32, device="cuda")
    calls = {
        "solutions": lambda: L.pcgrl_solutions_for_grids(h, n, g.data_ptr(), cap, moves.data_ptr(), length.data_ptr(),
                                                         dist_win.data_ptr(), sp),
        "stats": lambda: L.pcgrl_stats_for_grids_h(h, n, g.data_ptr(), stats.data_ptr(), sp),
    }
    times = {k: [] for k in calls}
    for k, call in calls.items():
        for _ in range(args.warmup):
            assert call() == 0
    for w in range(args.windows):
        for k, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / args.calls * 1e6)
    env.check_errors()
    assert torch.equal(length.clamp(min=0), stats[:, 5]) and torch.equal(dist_win, stats[:, 4])
    key = f"{name} 16x16@{n}"
    row = {k: {"mean": round(statistics.mean(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)} for k, t in times.items()}
    row["solved"] = int((length > 0).sum())
    row["solver_ran"] = int((length >= 0).sum())
    row["longest_solution"] = int(length.max())
    row["ratio"] = round(row["solutions"]["mean"] / row["stats"]["mean"], 2)
    result["us_per_call"][key] = row
    print(f"{key:34s} solutions {row['solutions']['mean']:10.2f} us (min {row['solutions']['min']:.2f} max {row['solutions']['max']:.2f})   "
          f"stats {row['stats']['mean']:10.2f} us (min {row['stats']['min']:.2f} max {row['stats']['max']:.2f})   x{row['ratio']}   "
          f"solver ran {row['solver_ran']} solved {row['solved']} longest {row['longest_solution']}", flush=True)
env.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
