#!/usr/bin/env python3
"""Per-launch time of pcgrl_step on the 3-D maze under narrow, turtle and wide: random actions, auto-reset, 7^3 at 1024
envs and 15^3 at the batch of bench.py's minecraft_3D_maze-narrow-15 (1024).

    python tools/reps3d_bench.py [--rounds 5] [--steps 1500] [--warmup 400] [--out profiles/reps3d.json]
    python tools/reps3d_bench.py --only turtle --shape 7 --rounds 1          # one kernel, for a kernel trace of its own

The three representations alternate inside one process and the whole cycle repeats `--rounds` times, so drift of the
machine shows up as spread inside each column instead of as a difference between columns.  A window is `--steps` launches
on one stream between two device synchronisations (host clock), after `--warmup` launches of the same engine.  Engines
live for the whole run: an env's episode phase differs between windows, as it does in training.
PCGRL_LIB selects another build of the library inside csrc/ (the parent commit's, for the narrow yardstick): narrow only.
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

from control_pcgrl_amd import VecPcgrlEnv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=1500)
ap.add_argument("--warmup", type=int, default=400)
ap.add_argument("--only", default=None, help="one representation")
ap.add_argument("--shape", type=int, default=None, help="7 or 15: one map size")
ap.add_argument("--actions", default="random", choices=["random", "noedit"],
                help="noedit: steps with change == 0 only -- turtle draws moves alone, narrow and wide write AIR everywhere (nothing "
                     "changes once the map is AIR; give --init-density 0)")
ap.add_argument("--init-density", type=float, default=None,
                help="reset to maps of this DIRT density (and random turtle positions) instead of the reset's own maps, whose density is "
                     "random per env; auto-reset is then off, so the maps keep evolving from there")
ap.add_argument("--out", default=None)
args = ap.parse_args()

reps = [args.only] if args.only else (["narrow"] if os.environ.get("PCGRL_LIB") else ["narrow", "turtle", "wide"])
sizes = [((7, 7, 7), 1024), ((15, 15, 15), 1024)]
if args.shape:
    sizes = [s for s in sizes if s[0][0] == args.shape]
sp = torch.cuda.current_stream().cuda_stream
result = {"method": "host clock around --steps pcgrl_step launches between device synchronisations, representations alternating, "
                    "rounds repeated in one process; random actions, auto-reset", "steps": args.steps, "warmup": args.warmup,
          "rounds": args.rounds, "actions": args.actions, "init_density": args.init_density, "library": os.environ.get("PCGRL_LIB", "this build"), "us_per_launch": {}}
for shape, n in sizes:
    envs, pools = {}, {}
    for rep in reps:
        e = VecPcgrlEnv("minecraft_3D_maze", rep, shape, n, seeds=np.arange(n), auto_reset=args.init_density is None)
        g = torch.Generator(device="cuda").manual_seed(1)
        if args.init_density is None:
            e.reset()
        else:
            grids = (torch.rand((n,) + shape, generator=g, device="cuda") < args.init_density).to(torch.uint8)
            pos = torch.stack([torch.randint(0, d, (n,), generator=g, device="cuda", dtype=torch.int32) for d in shape], 1)
            e.reset(init_grids=grids, init_pos=pos.contiguous())
        if args.actions == "noedit":
            pools[rep] = (torch.randint(0, 4, (256, n), generator=g, device="cuda", dtype=torch.int32) if rep == "turtle"
                          else (torch.arange(256 * n, device="cuda", dtype=torch.int32).reshape(256, n) % int(np.prod(shape)))
                          * (2 if rep == "wide" else 0))
        else:
            pools[rep] = torch.randint(0, e.num_actions, (256, n), generator=g, device="cuda", dtype=torch.int32)
        for k in range(args.warmup):
            e.step_raw(pools[rep][k % 256].data_ptr(), sp)
        envs[rep] = e
    torch.cuda.synchronize()
    times = {rep: [] for rep in reps}
    for r in range(args.rounds):
        for rep in reps:
            e, pool = envs[rep], pools[rep]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.steps):
                e.step_raw(pool[(k + 37 * r) % 256].data_ptr(), sp)
            torch.cuda.synchronize()
            times[rep].append((time.perf_counter() - t0) / args.steps * 1e6)
    key = "x".join(str(s) for s in shape) + f"@{n}"
    result["us_per_launch"][key] = {}
    for rep in reps:
        envs[rep].check_errors()
        t = times[rep]
        row = {"mean": round(statistics.mean(t), 2), "min": round(min(t), 2), "max": round(max(t), 2), "rounds": [round(x, 2) for x in t],
               "obs_MB_per_launch": round(n * float(np.prod(envs[rep].obs_shape)) / 1e6, 2)}
        result["us_per_launch"][key][rep] = row
        print(f"{key:16s} {rep:7s} mean {row['mean']:8.2f} us  min {row['min']:8.2f}  max {row['max']:8.2f}  obs {row['obs_MB_per_launch']} MB/launch",
              flush=True)
        envs[rep].close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
