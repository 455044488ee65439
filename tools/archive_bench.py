#!/usr/bin/env python3
"""Time per call of the quality-diversity grid archive (include/pcgrl_amd_archive.h) next to the same work done on the host
and written with torch on the device, all measured in the same run.

    python tools/archive_bench.py [--windows 5] [--calls 50] [--warmup 10] [--out profiles/archive_bench.json]

The archive is 100 x 100 over (emptiness, path-length) of Lode Runner, the maps are 8 x 12 with 8 tiles, a batch is 4 096.
A window is `--calls` calls on one stream between two device synchronisations (host clock), after `--warmup` calls; the rows
alternate inside one process and the cycle repeats `--windows` times (the method of tools/measures_bench.py).  The engine
calls are the C calls with outputs allocated once.

  (a) add_empty       pcgrl_archive_add of 4 096 candidates into an empty archive
  (b) add_half        the same into an archive whose image holds the elites of an earlier batch in about half of the cells
                      the candidates fall in
      Both restore the archive's image before every add (pcgrl_archive_import, timed alone as `restore`): the row is the
      window of restore + add minus the window of restore.
  (c) ask             pcgrl_archive_ask(4096)
  (d) generation      evaluate -> behaviour -> add -> ask on the device, the children fed back (stock Lode Runner levels to
                      start with); `evaluate_behaviour` is its first half alone
  (e) generation_host the same generation with the archive on the host: .cpu() of maps, objectives and behaviours, the
                      sequential numpy restatement (tests/archive_rules.py), numpy selection and mutation, the copy back
  (f) torch_add_*     the insertion written with torch on the same device: placement, scatter_reduce_(amax) on the keys,
                      scatter_reduce_(amin) on the indices for the tie, a masked scatter of the rows; restore timed and
                      subtracted the same way.  Its archive must equal the kernel's exactly."""
import argparse
import ctypes as C
import glob
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

import archive_rules as R  # noqa: E402
from control_pcgrl_amd import LodeRunnerEvaluator, archive_for  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--host-calls", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "archive_bench needs the GPU: a host run gives no time"
DEV = torch.device("cuda:0")
N, NAMES, RATE = 4096, ["emptiness", "path-length"], 0.01


def window(call, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


ev = LodeRunnerEvaluator((8, 12), device=DEV)
arc = archive_for(ev, NAMES)
L, h, sp = arc._L, arc._h, torch.cuda.current_stream(DEV).cuda_stream
dims, bounds, cells = arc.dims, arc.bounds, arc.n_cells

# candidates: the stock levels, mutated, with the behaviours spread over the grid so that the batch meets many cells
stock = np.concatenate([np.load(f)["grids"] for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "loderunner", "stock_*.npz")))])
rng = np.random.default_rng(35)
maps = stock[rng.integers(0, len(stock), 2 * N)]
maps = np.where(rng.random(maps.shape) < 0.05, rng.integers(0, 8, maps.shape), maps).astype(np.uint8)
beh = np.stack([(maps == 0).reshape(2 * N, -1).sum(1) / 96.0, rng.integers(0, 96, 2 * N).astype(np.float64)], 1)
obj = -rng.integers(0, 8, 2 * N).astype(np.float64) / 2
g_maps, g_obj, g_beh = (torch.as_tensor(x).to(DEV).contiguous() for x in (maps, obj, beh))
status = torch.empty(N, dtype=torch.uint8, device=DEV)
cell = torch.empty(N, dtype=torch.int32, device=DEV)
counts = torch.empty(4, dtype=torch.int32, device=DEV)
kids = torch.empty((N, 8, 12), dtype=torch.uint8, device=DEV)
parent = torch.empty(N, dtype=torch.int32, device=DEV)

empty = arc.state_dict()["image"].clone()
arc.add(g_maps[N:], g_obj[N:], g_beh[N:])  # the earlier batch
half = arc.state_dict()["image"].clone()
hdr = C.create_string_buffer(empty[:128].cpu().numpy().tobytes(), 128)
occupied_half = arc.stats().count
fall_in = len(np.unique(arc.cell_of(g_beh[:N]).cpu().numpy()))
met = int(arc.dense().occupied[arc.cell_of(g_beh[:N]).long().unique()].sum())


def restore(img):
    return lambda: L.pcgrl_archive_import(h, img.data_ptr(), img.numel(), hdr, sp)


def add():
    rc = L.pcgrl_archive_add(h, N, g_maps.data_ptr(), g_obj.data_ptr(), g_beh.data_ptr(), None, status.data_ptr(),
                             cell.data_ptr(), counts.data_ptr(), sp)
    assert rc == 0


def both(img):
    r = restore(img)
    return lambda: (r(), add())


def ask():
    assert L.pcgrl_archive_ask(h, N, 7, RATE, kids.data_ptr(), parent.data_ptr(), sp) == 0


# ---- (f) the insertion in torch -------------------------------------------------------------------------------------------
I64_MIN, BIG = -(1 << 63), 1 << 40
lo_t = torch.tensor([b[0] for b in bounds], dtype=torch.float64, device=DEV)
hi_t = torch.tensor([b[1] for b in bounds], dtype=torch.float64, device=DEV)
dims_f = torch.tensor(dims, dtype=torch.float64, device=DEV)
dims_i = torch.tensor(dims, dtype=torch.int64, device=DEV)
arange = torch.arange(N, dtype=torch.int64, device=DEV)


def tkey(x):
    b = (x + 0.0).view(torch.int64)
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF)  # signed and order-preserving; nothing maps to I64_MIN


class TorchArchive:
    """cells + 1 rows: the last row takes every masked-out write"""

    def __init__(self):
        self.obj = torch.zeros(cells + 1, dtype=torch.float64, device=DEV)
        self.beh = torch.zeros((cells + 1, 2), dtype=torch.float64, device=DEV)
        self.flag = torch.zeros(cells + 1, dtype=torch.bool, device=DEV)
        self.maps = torch.zeros((cells + 1, 96), dtype=torch.uint8, device=DEV)

    def tensors(self):
        return self.obj, self.beh, self.flag, self.maps

    def add(self, maps, obj, beh):
        b = torch.minimum(torch.maximum(beh, lo_t), hi_t)
        i = torch.minimum((((b - lo_t) / (hi_t - lo_t)) * dims_f).to(torch.int64), dims_i - 1)
        c = i[:, 0] * dims[1] + i[:, 1]
        key = tkey(obj)
        okey = torch.where(self.flag[:cells], tkey(self.obj[:cells]), I64_MIN)
        best = okey.clone().scatter_reduce_(0, c, key, "amax")
        eligible = (key == best[c]) & (key > okey[c])
        win = torch.full((cells,), BIG, dtype=torch.int64, device=DEV).scatter_reduce_(0, c, torch.where(eligible, arange, BIG), "amin")
        winner = eligible & (win[c] == arange)
        st = torch.where(winner, torch.where(self.flag[c], 1, 2), 0).to(torch.uint8)
        dst = torch.where(winner, c, cells)
        self.obj.scatter_(0, dst, obj)
        self.beh.index_copy_(0, dst, beh)
        self.maps.index_copy_(0, dst, maps.reshape(N, 96))
        self.flag.scatter_(0, dst, torch.ones_like(winner))
        self.flag[cells] = False
        return st, c


tarc = TorchArchive()
t_empty = [t.clone() for t in tarc.tensors()]
tarc.add(g_maps[N:], g_obj[N:], g_beh[N:])
t_half = [t.clone() for t in tarc.tensors()]


def t_restore(saved):
    return lambda: [t.copy_(s) for t, s in zip(tarc.tensors(), saved)]


def t_both(saved):
    r = t_restore(saved)
    return lambda: (r(), tarc.add(g_maps[:N], g_obj[:N], g_beh[:N]))


# the torch insertion equals the kernel's, from the empty archive and from the half-full one
for img, saved in ((empty, t_empty), (half, t_half)):
    both(img)()
    t_restore(saved)()
    st, c = tarc.add(g_maps[:N], g_obj[:N], g_beh[:N])
    d = arc.dense()
    assert torch.equal(st, status) and torch.equal(c.to(torch.int32), cell)
    assert torch.equal(d.occupied.bool(), tarc.flag[:cells]) and torch.equal(d.grids.reshape(cells, 96), tarc.maps[:cells])
    assert torch.equal(d.objectives.view(torch.int64), tarc.obj[:cells].view(torch.int64))
    assert torch.equal(d.behaviours.view(torch.int64), tarc.beh[:cells].view(torch.int64))
counts_empty = (both(empty)(), counts.cpu().tolist())[1]
counts_half = (both(half)(), counts.cpu().tolist())[1]

# ---- (d), (e) the generation ----------------------------------------------------------------------------------------------
state = {"kids": g_maps[:N].reshape(N, 8, 12).clone()}


def evaluate_behaviour(g):
    res = ev.evaluate(g, gold_cap=0)
    b = torch.stack([ev.measures(g, entropy=False).bc["emptiness"], res["stats"][:, 4]], 1)
    return -res["loss"], b


def generation():
    o, b = evaluate_behaviour(state["kids"])
    arc.add(state["kids"], o, b)
    arc.ask(N, seed=7, rate=RATE, out=(state["kids"], parent))


host = {"arc": R.SeqArchive(dims, bounds, (8, 12)), "kids": g_maps[:N].reshape(N, 8, 12).clone(), "rng": np.random.default_rng(7)}


def generation_host():
    o, b = evaluate_behaviour(host["kids"])
    m, o, b = host["kids"].cpu().numpy(), o.cpu().numpy(), b.cpu().numpy()
    a = host["arc"]
    a.add(m, o, b)
    occ = a.occupied()
    p = a.maps[occ[host["rng"].integers(0, len(occ), N)]]
    hit = host["rng"].random(p.shape) < RATE
    p = np.where(hit, (p + host["rng"].integers(1, 8, p.shape)) % 8, p).astype(np.uint8)
    host["kids"] = torch.as_tensor(p).to(DEV)


rows = {
    "restore": (restore(half), args.calls), "add_empty+restore": (both(empty), args.calls),
    "add_half+restore": (both(half), args.calls), "ask": (ask, args.calls),
    "torch_restore": (t_restore(t_half), args.calls), "torch_add_empty+restore": (t_both(t_empty), args.calls),
    "torch_add_half+restore": (t_both(t_half), args.calls),
    "evaluate_behaviour": (lambda: evaluate_behaviour(state["kids"]), max(1, args.calls // 5)),
    "generation": (generation, max(1, args.calls // 5)), "generation_host": (generation_host, args.host_calls),
}
times = {k: [] for k in rows}
restore(half)()
for k, (call, n_calls) in rows.items():
    for _ in range(min(args.warmup, n_calls)):
        call()
for w in range(args.windows):
    restore(half)()
    for k, (call, n_calls) in rows.items():
        times[k].append(window(call, n_calls))
arc.check_errors()
ev.check_errors()

out = {k: {"mean_us": round(statistics.mean(t), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2)} for k, t in times.items()}
mean = lambda k: statistics.mean(times[k])
result = {
    "method": "host clock around --calls calls between device synchronisations; rows alternate, windows repeated in one "
              "process; add rows = (restore + add) - restore of the same cycle",
    "calls": args.calls, "warmup": args.warmup, "windows": args.windows, "host_calls": args.host_calls,
    "archive": {"dims": list(dims), "bounds": [list(b) for b in bounds], "map_shape": [8, 12], "n_tiles": 8, "batch": N,
                "image_bytes": arc.state_bytes, "occupied_half": occupied_half, "cells_the_batch_falls_in": fall_in,
                "of_them_occupied_in_half": met, "counts_empty": counts_empty, "counts_half": counts_half},
    "windows_us": out,
    "rows_us": {
        "a_add_empty": round(mean("add_empty+restore") - mean("restore"), 2),
        "b_add_half": round(mean("add_half+restore") - mean("restore"), 2),
        "c_ask": round(mean("ask"), 2),
        "d_generation_device": round(mean("generation"), 2),
        "d_evaluate_behaviour_alone": round(mean("evaluate_behaviour"), 2),
        "e_generation_host_archive": round(mean("generation_host"), 2),
        "f_torch_add_empty": round(mean("torch_add_empty+restore") - mean("torch_restore"), 2),
        "f_torch_add_half": round(mean("torch_add_half+restore") - mean("torch_restore"), 2),
    },
    "host_archive_occupied_after": int(host["arc"].flag.sum()), "device_archive_occupied_after": arc.stats().count,
}
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
