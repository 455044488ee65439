#!/usr/bin/env python3
"""Time per call of pcgrl_smb_measures_for_grids and pcgrl_smb_diversity_for_grids at 4 096 stock 16 x 116 Mario maps, next to
the torch expression on the same device in the same run.

    python tools/smb_measures_bench.py [--windows 5] [--calls 50] [--warmup 10] [--out profiles/smb_measures_bench.json]

Cases: the measures per call; the diversity as one group of K = 4 096 and in 8 groups of K = 512.  A window is `--calls` calls
on one stream between two device synchronisations (host clock), after `--warmup` calls; the library calls and the torch
baseline alternate inside one process and the cycle repeats `--windows` times, so drift of the machine shows as spread inside a
column (the method of tools/measures_bench.py).  The library calls write into buffers allocated once.  The torch baseline is the
chunked expression (g[a:b, None] != g[None]).sum(-1) per group, over as many rows at a time as fit `--torch-bytes` of its
boolean intermediate (4 096 stock maps unchunked would be 31 GB of booleans); it covers every pair the library call covers,
and before the timing its matrix is compared with the library's for equality, group by group.

Bounds, computed the way DESIGN.md section 16 does.  Pairwise kernel: per 64 row maps x 1 column map x 1 word it issues P = 3
8-byte LDS reads (2 LDS cycles each) and 4 P VALU instructions (2 cycles each on one of 4 SIMDs), so a CU needs 2 P cycles per
unit; `bound_us` is units * 2 P / (256 CUs * 2.4 GHz) for the full square with every CU busy.  Measure kernel: per map and
64-cell chunk one wave issues 7 one-byte LDS reads (the cell, two mirror cells, four neighbours; 2 LDS cycles each) and 16
compare-ballot-popcounts, so a CU needs 14 cycles per chunk by the LDS count; `measures_bound_us` is maps * NW * 14 / (256 CUs
* 2.4 GHz).  `expected_us` is what DESIGN.md section 24 wrote down before the first run."""
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
from control_pcgrl_amd import SmbEvaluator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--torch-bytes", type=int, default=1 << 30)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "smb_measures_bench needs the GPU: a host run gives no time"

CUS, CLOCK = 256, 2.4e9
T, P = 7, 3
H, W, n = 16, 116, 4096
cells = H * W
NW = (cells + 63) // 64
# DESIGN.md section 24.4, written before the first run: the 16 x 16 three-plane figures of profiles/measures_bench.json scaled
# by the word count (diversity: 78.14 us per 4 096-map group * 29 / 4; 8 groups of 512: the 64 x 64 figure 225.48 us * 29 / 64;
# measures: the 64 x 64 figure 72.61 us * 29 / 64)
EXPECTED = {"measures": 32.9, "diversity K=4096": 566.5, "diversity K=512": 102.2}

sp = torch.cuda.current_stream().cuda_stream
ev = SmbEvaluator((H, W), "cuda:0", solver_power=1000, max_levels=1)
L = ev._L
grids = np.random.default_rng(1).integers(0, T, size=(n, H, W), dtype=np.uint8)
g = torch.as_tensor(grids, device="cuda").contiguous()
flat = g.view(n, cells)
counts = torch.empty((n, T), dtype=torch.int32, device="cuda")
match = torch.empty((n, 3), dtype=torch.int32, device="cuda")
ent = torch.empty(n, dtype=torch.float64, device="cuda")
forms = torch.empty((n, 5 + T), dtype=torch.float64, device="cuda")
tab = ev._entropy_table()
scratch = torch.empty(int(L.pcgrl_smb_diversity_scratch_bytes(H, W, n)) // 8, dtype=torch.int64, device="cuda")
near = torch.empty(n, dtype=torch.int32, device="cuda")
nidx = torch.empty(n, dtype=torch.int32, device="cuda")


def window(call, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def torch_pairs(K):
    """the chunked expression, every group: a list of [rows, K] blocks"""
    step = max(1, args.torch_bytes // (K * cells))
    out = []
    for lo in range(0, n, K):
        grp = flat[lo:lo + K]
        for a in range(0, K, step):
            out.append((grp[a:a + step, None] != grp[None]).sum(-1))
    return out


def stats(t):
    return {"mean_us": round(statistics.mean(t), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2)}


result = {"method": "host clock around --calls calls between device synchronisations; library calls and the chunked torch "
                    "expression alternate, windows repeated in one process; the torch matrix compared with the library's first",
          "maps": n, "shape": [H, W], "words_per_plane": NW, "calls": args.calls, "warmup": args.warmup,
          "windows": args.windows, "torch_bytes": args.torch_bytes, "expected_us": EXPECTED, "cases": {}}


def measures_call():
    return L.pcgrl_smb_measures_for_grids(H, W, n, g.data_ptr(), counts.data_ptr(), match.data_ptr(), forms.data_ptr(),
                                          ent.data_ptr(), tab.data_ptr(), sp)


for _ in range(args.warmup):
    assert measures_call() == 0
times = [window(measures_call, args.calls) for _ in range(args.windows)]
assert np.array_equal(counts.cpu().numpy(), mn.counts(grids, T))
assert np.array_equal(match[:64].cpu().numpy(), mn.matches(grids[:64], T))
row = {"measures": stats(times), "expected_us": EXPECTED["measures"],
       "measures_bound_us": round(n * NW * 14 / (CUS * CLOCK) * 1e6, 3)}
row["measures_maps_per_s"] = n / (row["measures"]["mean_us"] * 1e-6)
row["map_bytes_per_s"] = n * cells / (row["measures"]["mean_us"] * 1e-6)
result["cases"]["measures"] = row
print("measures", json.dumps(row), flush=True)

for K in (4096, 512):
    G = n // K
    sums = torch.empty(G, dtype=torch.int64, device="cuda")
    scores = torch.empty((G, 2), dtype=torch.float64, device="cuda")

    def diversity_call(pw=None):
        return L.pcgrl_smb_diversity_for_grids(H, W, n, g.data_ptr(), K, scratch.data_ptr(), sums.data_ptr(), scores.data_ptr(),
                                               near.data_ptr(), nidx.data_ptr(), pw, sp)

    # equality first: the library's matrix against the torch expression's, every group
    pw = torch.empty((G, K, K), dtype=torch.int32, device="cuda")
    assert diversity_call(pw.data_ptr()) == 0
    want = torch.cat(torch_pairs(K)).view(G, K, K)
    assert torch.equal(pw.long(), want.long()), "the library's matrix differs from the torch expression's"
    assert torch.equal(sums, want.sum((1, 2), dtype=torch.int64))
    off = want.long() + torch.eye(K, dtype=torch.int64, device="cuda")[None] * (cells + 1)
    assert torch.equal(near.long(), off.min(2).values.reshape(-1))
    assert torch.equal(torch.gather(want.long(), 2, nidx.view(G, K, 1).long()).reshape(-1), near.long())
    assert int(sums[0]) == mn.hamming_sum(grids[:K], T)
    del pw, want, off
    calls = {"diversity": diversity_call, "torch_pairs": lambda: torch_pairs(K)}
    n_calls = {"diversity": args.calls, "torch_pairs": max(1, args.calls // 25)}
    times = {k: [] for k in calls}
    for k, call in calls.items():
        for _ in range(args.warmup if k == "diversity" else 1):
            call()
    for w in range(args.windows):
        for k, call in calls.items():
            times[k].append(window(call, n_calls[k]))
    pairs = G * K * K
    units = pairs * NW / 64
    row = {k: stats(t) for k, t in times.items()}
    row["pairs"] = pairs
    col_tiles, row_wgs = (K + 15) // 16, G * ((K + 63) // 64)
    tiles_per_split = -(-col_tiles // min(max(-(-2048 // row_wgs), 1), col_tiles))
    row["workgroups"] = row_wgs * -(-col_tiles // tiles_per_split)
    row["expected_us"] = EXPECTED[f"diversity K={K}"]
    row["bound_us"] = round(units * 2 * P / (CUS * CLOCK) * 1e6, 3)
    row["torch_over_diversity"] = round(row["torch_pairs"]["mean_us"] / row["diversity"]["mean_us"], 1)
    row["pairs_per_s"] = {"diversity": pairs / (row["diversity"]["mean_us"] * 1e-6),
                          "torch_pairs": pairs / (row["torch_pairs"]["mean_us"] * 1e-6)}
    result["cases"][f"diversity K={K}"] = row
    print(f"diversity K={K}", json.dumps(row), flush=True)

ev.check_errors()
ev.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
