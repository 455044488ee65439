"""Times Nca3dGenerator.generate against the torch formulation of the same roll-out on one MI355X -> profiles/nca3d_bench.json.

    python tools/nca3d_bench.py [--out profiles/nca3d_bench.json] [--reps 5] [--torch-chunk 256] [--no-torch]

Cases: the stock case of the reference's 3-D evolution (the holey dungeon: T = 5, 7 x 7 x 7, 4096 genomes x 10 seeds x 10
steps), the holey maze (T = 2) on the same map, and T = 2 on 15 x 15 x 15 with 256 genomes.  The torch side is what a population
on the device has to do without this kernel, in the same run on the same device: conv3d(groups=G) per layer on the one-hot
bordered map (genomes in chunks of --torch-chunk, so that the activations fit; no padding, so that the interior alone comes
out), sigmoid, argmax, compare, all n_steps steps (it cannot stop a pair early).  torch sums in another order, so the share of
final maps on which the two agree is reported, not asserted.
The FLOP count is what the stated arithmetic does on the steps actually taken: 864 adds, 2 * 1024 and 2 * 32 T multiplies and
adds per cell and step; the sigmoids are not counted.  The peak it is set against is the fp32 vector rate without fused
multiply-add, 78.6 Top/s (half of the 157.3 TFLOP/s that counts an FMA as two).  The file is rewritten after every case.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from control_pcgrl_amd import Nca3dGenerator, fixed_holes, nca3d  # noqa: E402

DEV = "cuda:0"
PEAK_NO_FMA = 78.6e12
CASES = [("holey dungeon 7x7x7 (stock)", 5, (7, 7, 7), 4096, 10, 10), ("holey maze 7x7x7", 2, (7, 7, 7), 4096, 10, 10),
         ("holey maze 15x15x15", 2, (15, 15, 15), 256, 10, 10)]


def genomes(rng, G, T):
    out = np.empty((G, nca3d.n_params(T)), np.float32)
    for g in range(G):
        w = nca3d.unpack_weights(out[g], T)
        for m, fan in ((w.w1, 27 * T), (w.w2, 32), (w.w3, 32)):
            m[...] = rng.normal(0, 2.0 / np.sqrt(fan), m.shape)
        for b in (w.b1, w.b2, w.b3):
            b[...] = rng.normal(0, 0.1, b.shape)
    return out


def torch_rollout(weights, init, holes, T, n_steps, chunk):
    """conv3d(groups=G) per layer on the bordered map, argmax, compare: the final interiors [G, S, D0, D1, D2] and whether each
    pair's map still changed at the last step"""
    G, P = weights.shape
    S, D0, D1, D2 = init.shape
    finals = []
    o = [0, 864 * T, 864 * T + 32, 864 * T + 32 + 1024, 864 * T + 32 + 1056, 864 * T + 32 + 1056 + 32 * T, P]
    for a in range(0, G, chunk):
        w = weights[a:a + chunk]
        g = w.shape[0]
        w1, b1 = w[:, o[0]:o[1]].reshape(g * 32, T, 3, 3, 3), w[:, o[1]:o[2]].reshape(g * 32)
        w2, b2 = w[:, o[2]:o[3]].reshape(g * 32, 32, 1, 1, 1), w[:, o[3]:o[4]].reshape(g * 32)
        w3, b3 = w[:, o[4]:o[5]].reshape(g * T, 32, 1, 1, 1), w[:, o[5]:o[6]].reshape(g * T)
        seen = torch.ones((S, g, D0 + 2, D1 + 2, D2 + 2), dtype=torch.uint8, device=weights.device)  # the border: DIRT
        for z, y, x in holes.tolist():
            seen[:, :, z:z + 2, y, x] = 0  # foot and head: AIR
        m = init[:, None].expand(S, g, D0, D1, D2).contiguous()
        for _ in range(n_steps):
            seen[:, :, 1:-1, 1:-1, 1:-1] = m
            x = F.one_hot(seen.long(), T).permute(0, 1, 5, 2, 3, 4).reshape(S, g * T, D0 + 2, D1 + 2, D2 + 2).float()
            x = torch.relu(F.conv3d(x, w1, b1, groups=g))
            x = torch.relu(F.conv3d(x, w2, b2, groups=g))
            x = torch.sigmoid(F.conv3d(x, w3, b3, groups=g))
            nxt = x.reshape(S, g, T, D0, D1, D2).argmax(dim=2).to(torch.uint8)
            changed = (nxt != m).flatten(2).any(dim=2)  # (the compare of the reference's loop; nothing can act on it here)
            m = nxt
        finals.append(m.permute(1, 0, 2, 3, 4))
    return torch.cat(finals), changed


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times)), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nca3d_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-chunk", type=int, default=256)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    rows = []
    for name, T, shape, G, S, n_steps in CASES:
        rng = np.random.default_rng(2024)
        w = torch.as_tensor(genomes(rng, G, T)).to(DEV)
        init = torch.as_tensor(rng.integers(0, T, size=(S,) + shape).astype(np.uint8)).to(DEV)
        holes = torch.as_tensor(fixed_holes(shape)).to(DEV)
        gen = Nca3dGenerator(T, shape, n_steps=n_steps, holey=True, device=DEV)
        out = gen.generate(w, init, holes=holes)
        t_kernel, all_k = timed(lambda: gen.generate(w, init, holes=holes, out=out), args.reps)
        gen.check_errors()
        steps = int((out.n_step.long() + 1).sum())
        cells = shape[0] * shape[1] * shape[2]
        ops = steps * cells * (864 + 2 * 1024 + 2 * 32 * T)
        row = {"case": name, "n_tiles": T, "map": list(shape), "genomes": G, "seeds": S, "n_steps": n_steps,
               "kernel_s": t_kernel, "kernel_all_s": all_k, "steps_taken": steps,
               "share_of_steps_saved_by_early_stops": 1.0 - steps / (G * S * n_steps),
               "pairs_stopped_early": int((out.n_step < n_steps - 1).sum()),
               "ps_per_cell_step_taken": t_kernel / (steps * cells) * 1e12, "ops": ops, "ops_per_s": ops / t_kernel,
               "share_of_fp32_vector_peak_without_fma": ops / t_kernel / PEAK_NO_FMA}
        print(json.dumps(row), flush=True)
        if not args.no_torch:
            t0 = time.time()
            ref, _ = torch_rollout(w, init, holes, T, n_steps, args.torch_chunk)
            torch.cuda.synchronize()
            print(f"torch first call {time.time() - t0:.1f} s", flush=True)
            t_torch, all_t = timed(lambda: torch_rollout(w, init, holes, T, n_steps, args.torch_chunk), 2)
            agree = (ref == out.levels).flatten(2).all(dim=2).float().mean().item()
            row.update({"torch_s": t_torch, "torch_all_s": all_t, "torch_chunk": args.torch_chunk, "torch_over_kernel":
                        t_torch / t_kernel, "final_maps_agreeing_with_torch": agree})
            print(json.dumps(row), flush=True)
        rows.append(row)
        gen.close()
        result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": rows}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
