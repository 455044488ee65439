#!/usr/bin/env python3
"""Time per call of pcgrl_measures_for_grids and pcgrl_diversity_for_grids next to two baselines measured in the same run: the
torch expression on the device and numpy on the host.

    python tools/measures_bench.py [--windows 5] [--calls 50] [--warmup 10] [--out profiles/measures_bench.json]

Cases: 4 096 zelda maps of 16 x 16 in groups of K = 64 and as one group of K = 4 096, and 4 096 maps of 64 x 64 in groups of
K = 512 (three bit-planes: the larger distance kernel).  A window is `--calls` calls on one stream between two device
synchronisations (host clock), after `--warmup` calls; the engine call and the torch baseline alternate inside one process
and the cycle repeats `--windows` times, so drift of the machine shows as spread inside a column.  The engine calls write into
buffers allocated once.  The torch baseline is (g[:, None] != g[None]).sum(-1) per group, over as many groups at a time as
fit `--torch-bytes` of its boolean intermediate (and over fewer maps than the engine where the whole batch would take too
long: the row says how many); numpy runs the same expression on the host once, on a subset, and both are scaled to the
engine's pair count in `pairs_per_s`.

The pairwise kernel's own bound: per 64 row maps x 1 column map x 1 word it issues P 8-byte LDS reads
(2 LDS cycles each) and 4 P VALU instructions (2 xor and 2 or per plane less one or pair, 2 popcount-adds; 2 cycles each on
one of 4 SIMDs), so a CU needs max(2 P, 2 P) = 2 P cycles per unit; `bound_us` is units * 2 P / (256 CUs * 2.4 GHz) for the
full square with every CU busy; `workgroups` is the number of one-wave workgroups the call launches (256 CUs x 4 SIMDs)."""
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

import measures_numpy as mn  # noqa: E402
from control_pcgrl_amd import VecPcgrlEnv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--torch-bytes", type=int, default=1 << 30)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "measures_bench needs the GPU: a host run gives no time"

CUS, CLOCK = 256, 2.4e9
CASES = [("zelda", (16, 16), 4096, 64), ("zelda", (16, 16), 4096, 4096), ("zelda", (64, 64), 4096, 512),
         ("binary", (16, 16), 4096, 64), ("binary", (64, 64), 4096, 512)]
sp = torch.cuda.current_stream().cuda_stream
result = {"method": "host clock around --calls calls between device synchronisations; engine calls and the torch expression "
                    "alternate, windows repeated in one process; numpy once on a subset",
          "calls": args.calls, "warmup": args.warmup, "windows": args.windows, "cases": {}}


def window(call, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


for problem, shape, n, K in CASES:
    T = mn.N_TILES[problem]
    P = mn.n_planes(T)
    cells = shape[0] * shape[1]
    NW = (cells + 63) // 64
    env = VecPcgrlEnv(problem, "narrow", shape, 4)
    L, h = env._L, env._h
    grids = np.random.default_rng(1).integers(0, T, size=(n,) + shape, dtype=np.uint8)
    g = torch.as_tensor(grids, device="cuda").contiguous()
    G = n // K
    counts = torch.empty((n, T), dtype=torch.int32, device="cuda")
    match = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    ent = torch.empty(n, dtype=torch.float64, device="cuda")
    forms = torch.empty((n, 5 + T), dtype=torch.float64, device="cuda")
    scores = torch.empty((n // K, 2), dtype=torch.float64, device="cuda")
    tab = env._entropy_table()
    scratch = torch.empty(int(L.pcgrl_diversity_scratch_bytes(h, n)) // 8, dtype=torch.int64, device="cuda")
    sums = torch.empty(G, dtype=torch.int64, device="cuda")
    near = torch.empty(n, dtype=torch.int32, device="cuda")
    nidx = torch.empty(n, dtype=torch.int32, device="cuda")
    # the torch expression: groups per slice so that the boolean intermediate [slice, K, K, cells] fits
    n_torch = n if K * cells <= (1 << 20) else min(n, 2 * K)  # (a 4 096-map group of 16 x 16 is 4 GB of booleans per slice)
    per = max(1, args.torch_bytes // (K * K * cells))
    rows = max(1, args.torch_bytes // (K * cells))  # K > per-slice budget: rows of one group at a time
    gt = g[:n_torch].view(n_torch // K, K, cells)

    def torch_pairs():
        out = []
        if K * K * cells <= args.torch_bytes:
            for s in range(0, gt.shape[0], per):
                x = gt[s:s + per]
                out.append((x[:, :, None] != x[:, None]).sum(-1))
        else:
            for grp in gt:
                for r in range(0, K, rows):
                    out.append((grp[r:r + rows, None] != grp[None]).sum(-1))
        return out

    calls = {
        "measures": lambda: L.pcgrl_measures_for_grids(h, n, g.data_ptr(), counts.data_ptr(), match.data_ptr(), forms.data_ptr(),
                                                       ent.data_ptr(), tab.data_ptr(), sp),
        "diversity": lambda: L.pcgrl_diversity_for_grids(h, n, g.data_ptr(), K, scratch.data_ptr(), sums.data_ptr(),
                                                         scores.data_ptr(), near.data_ptr(), nidx.data_ptr(), None, sp),
        "torch_pairs": torch_pairs,
    }
    n_calls = {"measures": args.calls, "diversity": args.calls, "torch_pairs": max(1, args.calls // 10)}
    times = {k: [] for k in calls}
    for k, call in calls.items():
        for _ in range(max(1, args.warmup if k != "torch_pairs" else 2)):
            call()
    for w in range(args.windows):
        for k, call in calls.items():
            times[k].append(window(call, n_calls[k]))
    env.check_errors()
    # the results of the timed calls are the rules' (a subset on the host)
    if K * K * cells <= 1 << 28:
        sub = min(G, 2)
        S, nn, ni, _ = mn.diversity(grids[:sub * K], T, K)
        assert np.array_equal(sums[:sub].cpu().numpy(), S) and np.array_equal(near[:sub * K].cpu().numpy(), nn)
        assert np.array_equal(nidx[:sub * K].cpu().numpy(), ni)
    else:  # (no K x K x cells intermediate on the host: the histogram identity)
        assert int(sums[0]) == mn.hamming_sum(grids[:K], T)
    assert np.array_equal(counts.cpu().numpy(), mn.counts(grids, T))
    # numpy on the host, once, on at most 256 maps of one group
    kn = min(K, 256)
    t0 = time.perf_counter()
    mn.pairwise(grids[:kn], T)
    numpy_us = (time.perf_counter() - t0) * 1e6
    pairs = G * K * K
    units = pairs * NW / 64
    row = {k: {"mean_us": round(statistics.mean(t), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2)}
           for k, t in times.items()}
    row["pairs"] = pairs
    row["torch_maps"] = n_torch
    # the engine's split of a group's columns (div_splits, measures/pcgrl_measures.h): about 2 048 one-wave workgroups
    col_tiles, row_wgs = (K + 15) // 16, G * ((K + 63) // 64)
    tiles_per_split = -(-col_tiles // min(max(-(-2048 // row_wgs), 1), col_tiles))
    row["workgroups"] = row_wgs * -(-col_tiles // tiles_per_split)
    row["bound_us"] = round(units * 2 * P / (CUS * CLOCK) * 1e6, 3)
    row["pairs_per_s"] = {"diversity": pairs / (row["diversity"]["mean_us"] * 1e-6),
                          "torch_pairs": (n_torch // K) * K * K / (row["torch_pairs"]["mean_us"] * 1e-6),
                          "numpy": kn * kn / (numpy_us * 1e-6)}
    row["measures_maps_per_s"] = n / (row["measures"]["mean_us"] * 1e-6)
    key = f"{problem} {shape[0]}x{shape[1]}@{n} K={K}"
    result["cases"][key] = row
    print(key, json.dumps(row), flush=True)
    env.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
