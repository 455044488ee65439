#!/usr/bin/env python3
"""What a `vector_step` of SmbVectorEnv costs per call against what the parent commit offers for the same result (DESIGN.md
section 23), on stock-size (16 x 116, window 32 x 232) turtle envs at solver_power 10000, for N = 20 (the reference's envs per
worker) and N = 4096.

    python tools/smb_vector_bench.py --envs 20 4096 --steps 1500 40 --out profiles/smb_vector_bench.json

    variants  adapter_f32 (no controls), adapter_f32_k2 (controls jumps, sol-length), adapter_u8 (no controls), and the baseline
              timed in the same run: SmbVecEnv.step -> the torch expression that builds the float32 image with the control
              planes in front -> .cpu(), without controls (baseline) and with the two (baseline_k2).
    starts    floor: an empty map and moves only -- no env ever searches, so the hand-out is what is timed; reset: the first
              `--steps` steps from a seeded reset with random actions (searches included; a finished env is reset as RLlib does).
    window    `--steps` calls (one number per size: the small size takes many, so that a window is not a few tens of
              milliseconds), each ending with its result on the host (the adapter waits for its stream, .cpu() waits for its
              copy), on the host clock, after `--warmup` calls from the same start; the variants alternate and the cycle repeats
              `--windows` times.  Per variant the median and the spread (max - min) of its windows; the ratio is baseline
              median over adapter median, per start and N.
    outputs   before anything is timed, at each size and from each start, the adapter's observations, float64 rewards, dones and
              statistics of three steps are compared with the baseline's, exactly.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="*", default=[20, 4096])
ap.add_argument("--steps", type=int, nargs="*", default=[1500, 40], help="per entry of --envs (the last one repeats)")
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
H, W, POWER, DEV = 16, 116, 10000, "cuda:0"
CTRL2 = ["jumps", "sol-length"]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from control_pcgrl_amd import SmbVecEnv, SmbVectorEnv  # noqa: E402

assert torch.cuda.is_available(), "smb_vector_bench needs the GPU: a host run gives no time"
WU = args.warmup


class Baseline:
    """the parent commit's pieces composed: the uint8 step, the float32 image with the control planes in front, the copy"""

    def __init__(self, vec):
        self.vec = vec

    def _image(self, obs):
        o = obs.float()
        c = self.vec.ctrl_obs
        if c is not None:
            o = torch.cat((c[:, None, None, :].expand(o.shape[:-1] + (c.shape[1],)), o), dim=-1)
        return o.cpu()

    def start(self, grids):
        self.vec.seed(np.arange(self.vec.num_envs))
        self._image(self.vec.reset(init_grids=grids)[0])

    def step(self, a_np, a_dev):
        obs, rew, done, _, info = self.vec.step(a_dev)
        out = self._image(obs), rew.cpu(), done.cpu(), info["stats"].cpu()
        if bool(out[2].any()):
            self._image(self.vec.reset(mask=done)[0])
        return out


class Adapter:
    def __init__(self, vec, obs_dtype):
        self.ad = SmbVectorEnv(vec=vec, obs_dtype=obs_dtype)
        self.vec = vec

    def start(self, grids):
        self.vec.seed(np.arange(self.vec.num_envs))
        if grids is None:
            self.ad.vector_reset()
        else:  # (the adapter resets by drawing; an injected start goes through the env, the hand-out is the same)
            self.vec.reset(init_grids=grids)
            self.ad._pending[:] = False

    def step(self, a_np, a_dev):
        out = self.ad.vector_step(a_np)
        if any(out[2]):
            for i in np.nonzero(out[2])[0]:
                self.ad.reset_at(int(i))
        return out


def window(v, grids, acts_np, acts_dev):
    T = len(acts_np) - WU
    v.start(grids)
    for t in range(WU):
        v.step(acts_np[t], acts_dev[t])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(WU, WU + T):
        v.step(acts_np[t], acts_dev[t])
    torch.cuda.synchronize()
    v.vec.check_errors()
    return round((time.perf_counter() - t0) / T * 1e6, 2)


def same_results(a, b, grids, acts_np, acts_dev):
    """three steps of adapter a and baseline b from the same start: everything handed out is equal, exactly"""
    a.start(grids)
    b.start(grids)
    for t in range(3):
        obs, rew, done, _, infos = a.step(acts_np[t], acts_dev[t])
        bobs, brew, bdone, bstats = b.step(acts_np[t], acts_dev[t])
        assert np.array_equal(np.stack(obs), bobs.numpy()), "observations differ"
        assert rew == brew.tolist() and done == bdone.tolist(), "rewards or dones differ"
        assert np.array_equal(a.ad._stats, bstats.numpy()), "statistics differ"
    return True


result = {"what": "tools/smb_vector_bench.py: per-call vector_step of SmbVectorEnv against SmbVecEnv.step -> float32 image with "
                  "control planes (torch) -> .cpu(), microseconds per call on the host clock, every call ending on the host",
          "map_shape": [H, W], "obs_window": [2 * H, 2 * W], "solver_power": POWER, "warmup": WU,
          "windows": args.windows, "sizes": {}}
for j, n in enumerate(args.envs):
    T = args.steps[min(j, len(args.steps) - 1)]
    rng = np.random.default_rng(11 + n)

    def vec(controls):
        return SmbVecEnv("turtle", (H, W), n, device=DEV, solver_power=POWER, seeds=np.arange(n), auto_reset=False,
                         reward_dtype=torch.float64, controls=controls)

    variants = {"adapter_f32": Adapter(vec(None), np.float32), "adapter_f32_k2": Adapter(vec(CTRL2), np.float32),
                "adapter_u8": Adapter(vec(None), np.uint8), "baseline": Baseline(vec(None)), "baseline_k2": Baseline(vec(CTRL2))}
    empty = torch.zeros((n, H, W), dtype=torch.uint8, device=DEV)
    starts = {"floor": (empty, rng.integers(0, 4, (T + WU, n))), "reset": (None, rng.integers(0, 11, (T + WU, n)))}
    size = {"steps": T, "direct_host_outputs": {k: v.ad._direct for k, v in variants.items() if isinstance(v, Adapter)},
            "bytes_per_call": {k: v.ad._total for k, v in variants.items() if isinstance(v, Adapter)}, "starts": {}}
    for s, (grids, acts) in starts.items():
        acts_dev = torch.as_tensor(acts, dtype=torch.int32, device=DEV)
        acts_np = [a.tolist() for a in acts]
        size.setdefault("outputs_equal_baseline", {})[s] = {
            k: same_results(variants[k], variants[b], grids, acts_np, acts_dev)
            for k, b in (("adapter_f32", "baseline"), ("adapter_f32_k2", "baseline_k2"))}
        print("outputs", n, s, size["outputs_equal_baseline"][s], flush=True)
        times = {k: [] for k in variants}
        for w in range(args.windows):
            for k, v in variants.items():
                times[k].append(window(v, grids, acts_np, acts_dev))
                print("window", n, s, w, k, times[k][-1], "us", flush=True)
        med = {k: statistics.median(t) for k, t in times.items()}
        size["starts"][s] = {
            "variants": {k: {"windows_us": t, "median_us": round(med[k], 2), "spread_us": round(max(t) - min(t), 2)}
                         for k, t in times.items()},
            "ratio_baseline_over_adapter_f32": round(med["baseline"] / med["adapter_f32"], 3),
            "ratio_baseline_k2_over_adapter_f32_k2": round(med["baseline_k2"] / med["adapter_f32_k2"], 3),
            "ratio_adapter_f32_over_adapter_u8": round(med["adapter_f32"] / med["adapter_u8"], 3)}
    result["sizes"][str(n)] = size
    for v in variants.values():
        v.vec.close()
    del variants
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
