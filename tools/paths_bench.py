#!/usr/bin/env python3
"""Time per call of pcgrl_paths_for_grids next to pcgrl_stats_for_grids_h on the same maps: binary and zelda, 4 096 maps at
16 x 16 and 1 024 at 64 x 64, maps of random density and all-passable maps.

    python tools/paths_bench.py [--windows 5] [--calls 200] [--warmup 50] [--out profiles/paths_bench.json]

The method of tools/reps3d_bench.py: a window is `--calls` calls on one stream between two device synchronisations (host
clock), after `--warmup` calls; the two entry points alternate inside one process and the cycle repeats `--windows` times,
so drift of the machine shows up as spread inside a column instead of as a difference between columns.  Both write into
buffers allocated once.  The path call runs with the default capacity (n_cells / 2 * n_cells rows per map) and the overlay:
its stores are 1 KB (binary) or 2 KB (zelda) of cells plus 256 B of overlay per 16 x 16 map, against 8 / 28 B of statistics.
"""
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

import paths_numpy as pn  # noqa: E402
from control_pcgrl_amd import VecPcgrlEnv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--out", default=None)
args = ap.parse_args()

sp = torch.cuda.current_stream().cuda_stream
result = {"method": "host clock around --calls calls between device synchronisations, paths_for_grids (default cap, overlay) and "
                    "stats_for_grids alternating on the same maps, windows repeated in one process",
          "calls": args.calls, "warmup": args.warmup, "windows": args.windows, "us_per_call": {}}
for problem in ("binary", "zelda"):
    for shape, n in (((16, 16), 4096), ((64, 64), 1024)):
        env = VecPcgrlEnv(problem, "narrow", shape, 4)
        L, h = env._L, env._h
        cap = int(L.pcgrl_path_capacity(h))
        for maps in ("random", "open"):
            if maps == "random":
                grids = pn.random_maps(problem, n, shape, np.random.default_rng(1))
            else:  # all passable; zelda: the player, the key and the door in three corners
                grids = np.zeros((n,) + shape, np.uint8)
                if problem == "zelda":
                    grids[:, 0, 0], grids[:, -1, -1], grids[:, 0, -1] = pn.PLAYER, pn.KEY, pn.DOOR
            g = torch.as_tensor(grids, device="cuda").contiguous()
            coords = torch.empty((n, cap, 2), dtype=torch.int16, device="cuda")
            length = torch.empty(n, dtype=torch.int32, device="cuda")
            overlay = torch.empty((n,) + shape, dtype=torch.uint8, device="cuda")
            stats = torch.empty((n, env.n_stats), dtype=torch.int32, device="cuda")
            calls = {
                "paths": lambda: L.pcgrl_paths_for_grids(h, n, g.data_ptr(), cap, coords.data_ptr(), length.data_ptr(),
                                                         overlay.data_ptr(), sp),
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
            key = f"{problem} {shape[0]}x{shape[1]}@{n} {maps}"
            row = {k: {"mean": round(statistics.mean(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)} for k, t in times.items()}
            row["mean_path_cells"] = round(float(length.float().mean()), 1)
            row["longest_path"] = int(length.max())
            row["ratio"] = round(row["paths"]["mean"] / row["stats"]["mean"], 2)
            result["us_per_call"][key] = row
            print(f"{key:28s} paths {row['paths']['mean']:9.2f} us (min {row['paths']['min']:.2f} max {row['paths']['max']:.2f})   stats "
                  f"{row['stats']['mean']:9.2f} us (min {row['stats']['min']:.2f} max {row['stats']['max']:.2f})   x{row['ratio']}   "
                  f"cells mean {row['mean_path_cells']} longest {row['longest_path']}", flush=True)
        env.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
