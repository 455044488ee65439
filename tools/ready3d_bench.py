"""Asynchronous stepping of the 3-D maze (pcgrl_step_ready on resumable path searches, include/pcgrl_amd_async3d.h) against
synchronous stepping (pcgrl_step), on the same seeded workload.

  python tools/ready3d_bench.py [--out profiles/async3d_bench.json] [--repeats 3] [--only 7|15]
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ready3d_bench.py --profile-pass

Workloads (same seeds 0x5EED + i, same pre-drawn random action rows for every mode, auto-reset on):
  7^3   BASELINE config 5: minecraft_3D_maze narrow 7 x 7 x 7, 1024 envs; 400 warm-up launches (past the first board scan of
        343 steps), then repeats of 10 000 launches (5 replays of a 2000-launch graph).
  15^3  the reference's stock map, 256 envs, from a reset over one whole episode of pcgrl_step (10 126 launches) per repeat.
Modes, alternated repeat by repeat in ONE process: (a) pcgrl_step; (b) pcgrl_step_ready at budgets 1, 2, 4, 8, 16, 32, 64 and
1 << 20 (nothing parks: what the resumable kernels cost by themselves).  Every mode has an engine of its own and a captured
HIP graph of its launches (a chain of kernel nodes, one status row per launch); a repeat = the graph's replays, timed with device
events.  Reported per mode: us per launch, the share of env-launches that EMITTED a transition, emitted env-steps/s, each with
the spread (max - min) of the repeats.  bench.py is not involved."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from control_pcgrl_amd import VecPcgrlEnv  # noqa: E402

BUDGETS = [1, 2, 4, 8, 16, 32, 64, 1 << 20]
WORKLOADS = {
    "7": dict(shape=(7, 7, 7), envs=1024, warmup=400, graph_launches=2000, replays=5),
    # one episode = max_iterations + 1 = 3 * 15^3 + 1 steps; 5 replays of a 2026-launch graph (the action rows repeat)
    "15": dict(shape=(15, 15, 15), envs=256, warmup=0, graph_launches=2026, replays=5),
}


class Mode:
    def __init__(self, w, budget, acts):
        n = w["envs"]
        self.budget, self.n, self.w = budget, n, w
        self.env = VecPcgrlEnv("minecraft_3D_maze", "narrow", w["shape"], n, seeds=0x5EED + np.arange(n), auto_reset=True)
        if budget:
            self.env.set_solver_budget(budget)
        self.env.reset()
        self.status = torch.ones((w["graph_launches"], n), dtype=torch.uint8, device="cuda")  # (pcgrl_step: every env emits)
        self.acts = acts
        for t in range(w["warmup"]):
            self.launch(t % w["graph_launches"], torch.cuda.current_stream().cuda_stream)
        self.env.check_errors()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):
                cap = torch.cuda.current_stream().cuda_stream
                for t in range(w["graph_launches"]):
                    self.launch(t, cap)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.us, self.share, self.rate = [], [], []

    def launch(self, t, stream):
        a = self.acts[t].data_ptr()
        rc = self.env.step_ready_raw(a, self.status[t].data_ptr(), stream) if self.budget else self.env.step_raw(a, stream)
        assert rc == 0, rc

    def repeat(self):
        w = self.w
        ms, emitted = 0.0, 0
        for _ in range(w["replays"]):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            self.graph.replay()
            t1.record()
            t1.synchronize()
            ms += t0.elapsed_time(t1)
            emitted += int((self.status & 1).sum())
        launches = w["replays"] * w["graph_launches"]
        self.us.append(ms * 1e3 / launches)
        self.share.append(emitted / (launches * self.n))
        self.rate.append(emitted / (ms * 1e-3))

    def row(self):
        def med(v):
            return statistics.median(v)

        return {"mode": "pcgrl_step" if not self.budget else "pcgrl_step_ready", "budget": self.budget,
                "us_per_launch": round(med(self.us), 3), "us_per_launch_spread": round(max(self.us) - min(self.us), 3),
                "emitted_share": round(med(self.share), 5),
                "emitted_env_steps_per_s": round(med(self.rate)), "emitted_env_steps_per_s_spread": round(max(self.rate) - min(self.rate)),
                "us_per_launch_all": [round(x, 3) for x in self.us], "emitted_env_steps_per_s_all": [round(x) for x in self.rate]}


def run(name, repeats):
    w = WORKLOADS[name]
    g = torch.Generator().manual_seed(0xA3)
    acts = torch.randint(0, 2, (w["graph_launches"], w["envs"]), generator=g, dtype=torch.int32).cuda()
    modes = [Mode(w, b, acts) for b in [0] + BUDGETS]
    for _ in range(repeats):
        for m in modes:  # alternating: every mode once per round
            m.repeat()
    for m in modes:
        m.env.check_errors()
    rows = [m.row() for m in modes]
    sync, ready = rows[0], rows[1:]
    best = max(ready, key=lambda r: r["emitted_env_steps_per_s"])
    out = {"workload": f"minecraft_3D_maze-narrow {'x'.join(map(str, w['shape']))}", "envs": w["envs"], "warmup_launches": w["warmup"],
           "launches_per_repeat": w["graph_launches"] * w["replays"], "repeats": repeats,
           "park_bytes_per_env": int(modes[1].env._L.pcgrl_park_bytes_per_env(modes[1].env._h)), "rows": rows,
           "best_budget": best["budget"],
           "best_over_sync": round(best["emitted_env_steps_per_s"] / sync["emitted_env_steps_per_s"], 4),
           "bar_met": bool(best["emitted_env_steps_per_s"] - sync["emitted_env_steps_per_s"] > sync["emitted_env_steps_per_s_spread"])}
    for r in rows:
        print(json.dumps({k: r[k] for k in ("mode", "budget", "us_per_launch", "us_per_launch_spread", "emitted_share",
                                            "emitted_env_steps_per_s", "emitted_env_steps_per_s_spread")}), flush=True)
    print(json.dumps({k: out[k] for k in ("workload", "best_budget", "best_over_sync", "bar_met")}), flush=True)
    for m in modes:
        m.env.close()
    return out


def profile_pass():
    """eager launches and nothing else: synchronous, budget 8 and budget 1 << 20 at 7^3 (for a rocprofv3 run of its own)"""
    w = WORKLOADS["7"]
    g = torch.Generator().manual_seed(0xA3)
    acts = torch.randint(0, 2, (500, w["envs"]), generator=g, dtype=torch.int32).cuda()
    for budget in (0, 8, 1 << 20):
        n = w["envs"]
        env = VecPcgrlEnv("minecraft_3D_maze", "narrow", w["shape"], n, seeds=0x5EED + np.arange(n), auto_reset=True)
        if budget:
            env.set_solver_budget(budget)
        env.reset()
        for t in range(900):
            env.step_ready(acts[t % 500]) if budget else env.step(acts[t % 500])
        env.check_errors()
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "async3d_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    ap.add_argument("--profile-pass", action="store_true")
    a = ap.parse_args()
    if a.profile_pass:
        profile_pass()
        return
    res = {"device": torch.cuda.get_device_name(0), "budgets": BUDGETS,
           "workloads": [run(k, a.repeats) for k in ([a.only] if a.only else ["7", "15"])]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
