"""Throughput of MDungeonEvaluator.evaluate on one GPU, and the plain-Python rules' time per level on the same levels.

    python tools/mdungeon_bench.py --out profiles/mdungeon_bench.json        (on the GPU)

Cases, 4 096 stock levels (11 x 7, solver_power 5 000) each:
  random       solid 0.1, potion 0.03, treasure 0.06, goblin and ogre 0.08 each, the rest empty, then one player and one exit
               (tests/mdungeon_levels.py random_level): at the tile probabilities of MDungeonProblem._prob (solid 0.4) about
               one 11 x 7 level in fifty has one player, one exit and one region, and the case would time the map scans alone
  structured   walls every third row with one door each, items in the rooms, the player at the top and the exit at the bottom
               (rooms)
  unsolvable   the exit in a corner behind three diagonals of ogres, no potion on the map, ten treasures in the open rest: one
               region, so the solver runs; no route survives, and each of the four stages spends its whole budget on
               (position, treasures taken) states (checked: 4 x 5 000 iterations a level)
Per case the tool times `calls` evaluate() calls between two device synchronisations with the host clock, `windows` times,
after a warm-up of every case; the kernel alone is the time between two device events around one pcgrl_mdungeon_evaluate call
on prepared buffers (no allocation, no other kernel), averaged over `calls` calls.  The first levels of each case are checked
against tests/mdungeon_rules.py, which is also timed on them on one host core in the same run.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import mdungeon_levels as ML  # noqa: E402
import mdungeon_rules as R  # noqa: E402

N, H, W, POWER = 4096, 11, 7, 5000


def unsolvable(rng):
    m = np.zeros((H, W), np.uint8)
    for y in range(4):
        for x in range(4 - y):
            m[y, x] = ML.EXIT if x + y == 0 else ML.OGRE  # 5 -> 3 -> 1 -> 0 on the way in, and nothing heals
    free = [(y, x) for y in range(H) for x in range(W) if x + y > 4]
    pick = rng.permutation(len(free))
    m[free[pick[0]]] = ML.PLAYER
    for i in pick[1:11]:
        m[free[i]] = ML.TREASURE
    return m


def cases():
    rng = np.random.default_rng(8200)
    return {"random": np.stack([ML.random_level(rng, H, W) for _ in range(N)]),
            "structured": np.stack([ML.rooms(rng, H, W) for _ in range(N)]),
            "unsolvable": np.stack([unsolvable(rng) for _ in range(N)])}


def gpu(calls, windows, rules_levels):
    import torch
    from control_pcgrl_amd import MDungeonEvaluator, _lib
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = "cuda:0"
    ev = MDungeonEvaluator((H, W), dev, solver_power=POWER, max_levels=N)
    maps = cases()
    grids = {k: torch.from_numpy(v).to(dev) for k, v in maps.items()}
    out = {}
    for name, g in grids.items():  # results first: the first levels against the rules, and the rules' time on them
        got = ev.evaluate(g, move_cap=64)
        t0 = time.perf_counter()
        want = [R.outputs(m, POWER, 64) for m in maps[name][:rules_levels]]
        rules_s = (time.perf_counter() - t0) / rules_levels
        for i, (stats, moves, length, play) in enumerate(want):
            assert got["stats"][i].tolist() == stats and got["moves"][i].tolist() == moves, (name, i)
            assert int(got["length"][i]) == length and got["play"][i].tolist() == play, (name, i)
        play = got["play"].cpu().numpy()
        its = play[:, 1:5].sum(1)
        if name == "unsolvable":
            assert (play[:, 0] == 0).all() and (play[:, 1:5] == POWER).all()
        rules_its = sum(sum(w[3][1:5]) for w in want)
        out[name] = {"searched_fraction": float((play[:, 0] >= 0).mean()), "won_fraction": float((play[:, 0] > 0).mean()),
                     "iterations": {"mean": float(its.mean()), "max": int(its.max())},
                     "rules": {"levels": rules_levels, "seconds_per_level": rules_s, "iterations": int(rules_its),
                               "ns_per_iteration": rules_s * rules_levels / max(1, rules_its) * 1e9}}
        for _ in range(2):
            ev.evaluate(g)
        torch.cuda.synchronize()
    L = _lib.lib()
    stats = torch.empty((N, 11), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for name, g in grids.items():
        ms = []
        for _ in range(windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                ev.evaluate(g)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / calls * 1e3)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kernel = []
        for _ in range(calls):
            start.record()
            _lib.check(L.pcgrl_mdungeon_evaluate(C.byref(ev._cfg), N, g.data_ptr(), ev._workspace.data_ptr(), ev._workspace_bytes,
                                                 0, stats.data_ptr(), None, None, None, None, stream))
            end.record()
            torch.cuda.synchronize()
            kernel.append(start.elapsed_time(end))
        r = out[name]
        r.update({"ms_per_call": {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))},
                  "kernel_ms": {"mean": float(np.mean(kernel)), "min": float(np.min(kernel)), "max": float(np.max(kernel))},
                  "levels_per_s": N / (float(np.mean(ms)) * 1e-3)})
        r["ns_per_iteration"] = float(np.mean(kernel)) * 1e6 / (r["iterations"]["mean"] * N)
        r["ns_per_iteration_longest"] = float(np.mean(kernel)) * 1e6 / r["iterations"]["max"]
        r["speedup_over_rules_one_core"] = r["rules"]["seconds_per_level"] * r["levels_per_s"]
    ev.check_errors()
    return out, ev._workspace_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--rules-levels", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"method": "host clock around --calls evaluate() calls between device synchronisations, --windows windows per case "
                     "after a warm-up of every case; kernel_ms: device events around one pcgrl_mdungeon_evaluate call; rules on "
                     "one host core over --rules-levels levels per case in the same run",
           "levels": N, "map_shape": [H, W], "solver_power": POWER, "calls": a.calls, "windows": a.windows,
           "mapping": "one wave per level, search on lane 0"}
    res["cases"], res["workspace_bytes"] = gpu(a.calls, a.windows, a.rules_levels)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
