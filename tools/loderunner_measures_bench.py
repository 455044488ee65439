#!/usr/bin/env python3
"""Time per call of LodeRunnerEvaluator.measures / .diversity / .behaviour at 4 096 stock 8 x 12 Lode Runner maps (the random
kind of tests/loderunner_levels.py), next to the torch expression and to evaluate() alone on the same device in the same run.

    python tools/loderunner_measures_bench.py [--windows 5] [--calls 200] [--warmup 10]
                                              [--out profiles/loderunner_measures_bench.json]

Cases: measures() per call (and the C entry point alone on buffers allocated once); diversity() as one group of K = 4 096 and
in 8 groups of K = 512, each against the chunked torch expression (g[a:b, None] != g[None]).sum(-1) per group, over as many rows
at a time as fit `--torch-bytes` of its boolean intermediate, with the matrices compared for equality first, group by group;
behaviour(("symmetry", "path-length")) against evaluate(gold_cap=0) alone, so that what the behaviour vector adds to an
evaluation is a measured difference.  A window is `--calls` calls on one stream between two device synchronisations (host
clock), after `--warmup` calls; the cases that are compared alternate inside one process and the cycle repeats `--windows`
times, so drift of the machine shows as spread inside a column (the method of tools/smb_measures_bench.py).

Bounds, computed the way DESIGN.md sections 16 and 24 do.  Pairwise kernel: per 64 row maps x 1 column map x 1 word it issues
P = 3 8-byte LDS reads (2 LDS cycles each) and 4 P VALU instructions, so a CU needs 2 P cycles per unit; `bound_us` is
units * 2 P / (256 CUs * 2.4 GHz) for the full square with every CU busy.  Measure kernel: per map and 64-cell chunk one wave
issues 7 one-byte LDS reads (the cell, two mirror cells, four neighbours; 2 LDS cycles each) and 17 compare-ballot-popcounts,
so a CU needs 14 cycles per chunk by the LDS count; `measures_bound_us` is maps * NW * 14 / (256 CUs * 2.4 GHz), and
`measures_bytes` what the call reads and writes.  `expected_us` is what DESIGN.md section 27.4 wrote down before the first run."""
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

import loderunner_levels as LL  # noqa: E402
import measures_numpy as mn  # noqa: E402
from control_pcgrl_amd import LodeRunnerEvaluator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--torch-bytes", type=int, default=1 << 30)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "loderunner_measures_bench needs the GPU: a host run gives no time"

CUS, CLOCK = 256, 2.4e9
T, P = 8, 3
H, W, n = 8, 12, 4096
cells = H * W
NW = (cells + 63) // 64
# DESIGN.md section 27.4, written before the first run
EXPECTED = {"measures": 10.0, "diversity K=4096": 47.0, "diversity K=512": 16.0, "behaviour minus evaluate": 20.0}

sp = torch.cuda.current_stream().cuda_stream
ev = LodeRunnerEvaluator((H, W), "cuda:0", max_levels=n)
L = ev._L
grids = LL.batch("random", 7000, n, H, W)
assert grids.shape == (n, H, W) and grids.dtype == np.uint8 and grids.max() < T
g = torch.as_tensor(grids, device="cuda").contiguous()
flat = g.view(n, cells)
counts = torch.empty((n, T), dtype=torch.int32, device="cuda")
match = torch.empty((n, 3), dtype=torch.int32, device="cuda")
ent = torch.empty(n, dtype=torch.float64, device="cuda")
forms = torch.empty((n, 5 + T), dtype=torch.float64, device="cuda")
tab = ev._entropy_table()
scratch = torch.empty(int(L.pcgrl_loderunner_diversity_scratch_bytes(H, W, n)) // 8, dtype=torch.int64, device="cuda")
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


def alternate(calls, n_calls, warmup):
    """windows of each call in turn, the cycle repeated --windows times -> {name: [us per call]}"""
    times = {k: [] for k in calls}
    for k, call in calls.items():
        for _ in range(warmup[k]):
            call()
    for _ in range(args.windows):
        for k, call in calls.items():
            times[k].append(window(call, n_calls[k]))
    return times


result = {"method": "host clock around --calls calls between device synchronisations; the calls that are compared alternate, "
                    "windows repeated in one process; the torch matrix compared with the library's first",
          "maps": n, "shape": [H, W], "levels": "tests/loderunner_levels.py batch('random', 7000, 4096, 8, 12)",
          "words_per_plane": NW, "calls": args.calls, "warmup": args.warmup, "windows": args.windows,
          "torch_bytes": args.torch_bytes, "expected_us": EXPECTED, "cases": {}}


# ------------------------------------------------------------------------------------------------------------ measures
def measures_launch():
    return L.pcgrl_loderunner_measures_for_grids(H, W, n, g.data_ptr(), counts.data_ptr(), match.data_ptr(), forms.data_ptr(),
                                                 ent.data_ptr(), tab.data_ptr(), sp)


assert measures_launch() == 0
assert np.array_equal(counts.cpu().numpy(), mn.counts(grids, T))
assert np.array_equal(match.cpu().numpy(), mn.matches(grids, T))
calls = {"measures": lambda: ev.measures(g), "measures_launch": measures_launch}
times = alternate(calls, dict.fromkeys(calls, args.calls), dict.fromkeys(calls, args.warmup))
row = {k: stats(t) for k, t in times.items()}
row["expected_us"] = EXPECTED["measures"]
row["measures_bound_us"] = round(n * NW * 14 / (CUS * CLOCK) * 1e6, 3)
row["measures_bytes"] = n * (cells + T * 4 + 3 * 4 + (5 + T) * 8 + 8)
row["measures_maps_per_s"] = n / (row["measures"]["mean_us"] * 1e-6)
result["cases"]["measures"] = row
print("measures", json.dumps(row), flush=True)

# ----------------------------------------------------------------------------------------------------------- diversity
for K in (4096, 512):
    G = n // K
    # equality first: the library's matrix against the torch expression's, every group
    d = ev.diversity(g, group=K, pairwise=True)
    want = torch.cat(torch_pairs(K)).view(G, K, K)
    assert torch.equal(d.pairwise.long(), want.long()), "the library's matrix differs from the torch expression's"
    assert torch.equal(d.hamming_sum, want.sum((1, 2), dtype=torch.int64))
    off = want.long() + torch.eye(K, dtype=torch.int64, device="cuda")[None] * (cells + 1)
    assert torch.equal(d.nearest.long(), off.min(2).values.reshape(-1))
    assert torch.equal(torch.gather(want.long(), 2, d.nearest_idx.view(G, K, 1).long()).reshape(-1), d.nearest.long())
    assert int(d.hamming_sum[0]) == mn.hamming_sum(grids[:K], T)
    del d, want, off
    sums = torch.empty(G, dtype=torch.int64, device="cuda")
    scores = torch.empty((G, 2), dtype=torch.float64, device="cuda")

    def diversity_launch():
        return L.pcgrl_loderunner_diversity_for_grids(H, W, n, g.data_ptr(), K, scratch.data_ptr(), sums.data_ptr(),
                                                      scores.data_ptr(), near.data_ptr(), nidx.data_ptr(), None, sp)

    calls = {"diversity": lambda: ev.diversity(g, group=K), "diversity_launch": diversity_launch,
             "torch_pairs": lambda: torch_pairs(K)}
    n_calls = {"diversity": args.calls, "diversity_launch": args.calls, "torch_pairs": max(1, args.calls // 25)}
    times = alternate(calls, n_calls, {"diversity": args.warmup, "diversity_launch": args.warmup, "torch_pairs": 1})
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

# ----------------------------------------------------------------------------------------------------------- behaviour
names = ("symmetry", "path-length")
b = ev.behaviour(g, names)
e = ev.evaluate(g, gold_cap=0)
assert torch.equal(b[:, 1], e["stats"][:, 4]) and torch.equal(b[:, 0], ev.measures(g, entropy=False).bc["symmetry"])
calls = {"evaluate": lambda: ev.evaluate(g, gold_cap=0), "behaviour": lambda: ev.behaviour(g, names)}
times = alternate(calls, dict.fromkeys(calls, args.calls), dict.fromkeys(calls, args.warmup))
row = {k: stats(t) for k, t in times.items()}
row["names"] = list(names)
row["behaviour_minus_evaluate_us"] = round(row["behaviour"]["mean_us"] - row["evaluate"]["mean_us"], 2)
row["expected_added_us"] = EXPECTED["behaviour minus evaluate"]
result["cases"]["behaviour"] = row
print("behaviour", json.dumps(row), flush=True)

ev.check_errors()
ev.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
