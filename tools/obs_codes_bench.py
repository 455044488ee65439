"""The tile-code observation form against the one-hot one (obs_format="codes", include/pcgrl_amd_codes.h).

  python tools/obs_codes_bench.py [--out profiles/obs_codes.json] [--rounds 10]
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/obs_codes_bench.py --profile-pass

Measures, in one process:
  step      per-step time of VecPcgrlEnv.step() in both forms for the four GPU configs of BASELINE at their batch sizes: a
            20-step HIP graph captured per form, replays timed with device events, the forms alternated round by round after
            a warm-up (median over rounds).  Codes: 2-D = the step launch without an observation + the from-state encoder,
            3-D = the step into a one-hot scratch + the compress kernel.
  adapter   PcgrlVectorEnv.vector_step env-steps/s at 4096 binary-narrow envs, obs_dtype uint8, both forms alternated.
  rollout   peak device memory of a 128-step rollout(want_obs="all") of 4096 zelda-turtle envs in both forms, and the codes
            form's rollout(want_obs="all") (one-hot scratch + compress) against K x (step + encoder), 2-D configs.
--profile-pass: eager steps of every config in both forms and nothing else (for a separate rocprofv3 run).
bench.py is not involved."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from control_pcgrl_amd import PcgrlVectorEnv, VecPcgrlEnv  # noqa: E402

CONFIGS = [("binary", "narrow", (16, 16), 4096), ("zelda", "turtle", (16, 16), 4096), ("sokoban", "wide", (16, 16), 2048),
           ("minecraft_3D_maze", "narrow", (7, 7, 7), 1024)]
GRAPH_STEPS = 20


def _env(problem, rep, shape, n, fmt):
    return VecPcgrlEnv(problem, rep, shape, n, seeds=0x5EED + np.arange(n), obs_format=fmt)


def _graph(env, warm=40):
    """a captured GRAPH_STEPS-step closed random-action loop (device-side sampling + step)"""
    acts = env.sample_actions(1)
    for _ in range(warm):  # (sokoban: lets the solver pool grow outside the capture)
        env.sample_actions(1, out=acts)
        env.step(acts)
    env.check_errors()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for _ in range(GRAPH_STEPS):
                env.sample_actions(1, out=acts)
                env.step(acts)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return g


def _time_graph(g, reps=5):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        g.replay()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / (reps * GRAPH_STEPS)  # us per step


def bench_steps(rounds):
    out = []
    for problem, rep, shape, n in CONFIGS:
        envs = {f: _env(problem, rep, shape, n, f) for f in ("onehot", "codes")}
        graphs = {}
        for f, e in envs.items():
            e.reset()
            graphs[f] = _graph(e)
            _time_graph(graphs[f], 3)  # warm-up replays
        times = {f: [] for f in envs}
        for _ in range(rounds):
            for f in ("onehot", "codes"):
                times[f].append(_time_graph(graphs[f]))
        for e in envs.values():
            e.check_errors()
        row = {"config": f"{problem}-{rep} {'x'.join(map(str, shape))}", "envs": n,
               "onehot_bytes_per_env": int(np.prod(envs["onehot"].obs_shape)), "codes_bytes_per_env": int(np.prod(envs["codes"].obs_shape)),
               "onehot_us_per_step": round(statistics.median(times["onehot"]), 3), "codes_us_per_step": round(statistics.median(times["codes"]), 3),
               "onehot_us_all": [round(x, 3) for x in times["onehot"]], "codes_us_all": [round(x, 3) for x in times["codes"]]}
        row["speedup"] = round(row["onehot_us_per_step"] / row["codes_us_per_step"], 3)
        print(json.dumps({k: row[k] for k in ("config", "envs", "onehot_us_per_step", "codes_us_per_step", "speedup")}), flush=True)
        out.append(row)
        for e in envs.values():
            e.close()
        del graphs
    return out


def bench_adapter(rounds, calls=200, n=4096):
    cfg = {"task": {"problem": "binary", "map_shape": (16, 16)}, "representation": "narrow"}
    envs = {"onehot": PcgrlVectorEnv(cfg, num_envs=n, seeds=np.arange(n), obs_dtype=np.uint8),
            "codes": PcgrlVectorEnv(dict(cfg, obs_format="codes"), num_envs=n, seeds=np.arange(n), obs_dtype=np.uint8)}
    rng = np.random.default_rng(0)
    acts = [rng.integers(0, 2, n) for _ in range(calls)]
    for e in envs.values():
        e.vector_reset()
        for a in acts[:20]:
            e.vector_step(a)
    rates = {f: [] for f in envs}
    for _ in range(rounds):
        for f, e in envs.items():
            t = time.perf_counter()
            for a in acts:
                e.vector_step(a)  # (no reset_at: finished envs keep stepping, which does not change the call's cost)
            rates[f].append(n * calls / (time.perf_counter() - t))
    out = {"config": "binary-narrow 16x16", "envs": n, "obs_dtype": "uint8", "calls_per_round": calls,
           "onehot_env_steps_per_s": round(statistics.median(rates["onehot"])), "codes_env_steps_per_s": round(statistics.median(rates["codes"])),
           "onehot_bytes_per_call": envs["onehot"]._total, "codes_bytes_per_call": envs["codes"]._total}
    out["speedup"] = round(out["codes_env_steps_per_s"] / out["onehot_env_steps_per_s"], 3)
    print(json.dumps(out), flush=True)
    for e in envs.values():
        e.close()
    return out


def bench_rollout_memory(n=4096, k=128):
    out = {"config": "zelda-turtle 16x16", "envs": n, "steps": k, "want_obs": "all"}
    for f in ("onehot", "codes"):
        e = _env("zelda", "turtle", (16, 16), n, f)
        e.reset()
        acts = torch.randint(0, e.num_actions, (k, n), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = e.rollout(acts, want_obs="all")
        torch.cuda.synchronize()
        out[f"{f}_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        out[f"{f}_obs_bytes"] = int(res[0].numel())
        e.check_errors()
        del res
        e.close()
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    return out


def bench_rollout_all(rounds, k=32):
    """rollout(want_obs="all") in codes form as VecPcgrlEnv.rollout takes it (see _ROLLOUT_COMPRESS_MAX_CHANNELS) against
    K x (step launch without an observation + from-state encoder into row k), both from the same state"""
    from control_pcgrl_amd import _lib
    out = []
    for problem, rep, shape, n in CONFIGS[:3]:
        e = _env(problem, rep, shape, n, "codes")
        e.reset()
        sd = e.state_dict()
        acts = torch.randint(0, e.num_actions, (k, n), dtype=torch.int32, device="cuda")
        obs = torch.empty((k, n) + e.obs_shape, dtype=torch.uint8, device="cuda")
        rew = torch.empty((k, n), dtype=torch.float32, device="cuda")
        done = torch.empty((k, n), dtype=torch.uint8, device="cuda")
        stats = torch.empty((k, n, e.n_stats), dtype=torch.int32, device="cuda")

        def per_step():
            s = e._stream()
            for j in range(k):
                _lib.check(e._L.pcgrl_step(e._h, acts[j].data_ptr(), 1, None, rew[j].data_ptr(), done[j].data_ptr(),
                                           stats[j].data_ptr(), s), "pcgrl_step")
                _lib.check(e._L.pcgrl_observe_codes(e._h, obs[j].data_ptr(), s), "pcgrl_observe_codes")

        times = {"rollout": [], "per_step": []}
        for r in range(rounds + 1):
            for f, fn in (("rollout", lambda: e.rollout(acts, want_obs="all")), ("per_step", per_step)):
                e.load_state_dict(sd)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                if r:  # (round 0: warm-up)
                    times[f].append(t0.elapsed_time(t1) * 1e3 / k)
        e.check_errors()
        row = {"config": f"{problem}-{rep} {'x'.join(map(str, shape))}", "envs": n, "steps": k,
               "rollout_us_per_step": round(statistics.median(times["rollout"]), 3),
               "per_step_encode_us_per_step": round(statistics.median(times["per_step"]), 3)}
        print(json.dumps(row), flush=True)
        out.append(row)
        e.close()
    return out


def profile_pass(steps=50):
    for problem, rep, shape, n in CONFIGS:
        for f in ("onehot", "codes"):
            e = _env(problem, rep, shape, n, f)
            e.reset()
            acts = e.sample_actions(1)
            for _ in range(steps):
                e.sample_actions(1, out=acts)
                e.step(acts)
            e.check_errors()
            e.close()
    print("profile pass done", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_codes.json"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--profile-pass", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.profile_pass:
        profile_pass()
        return
    res = {"device": torch.cuda.get_device_name(0), "graph_steps": GRAPH_STEPS, "rounds": a.rounds,
           "step": bench_steps(a.rounds), "adapter": bench_adapter(max(3, a.rounds // 2)), "rollout_memory": bench_rollout_memory(),
           "rollout_all": bench_rollout_all(max(3, a.rounds // 2))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
