"""Throughput of Mc3dHoleyEvaluator.evaluate on one GPU, the plain-Python rules' time per level on the same levels, and the
reference's own get_stats on them (timed on a CPU machine that has the reference, kept as data).

    python tools/mc3d_holey_bench.py --out profiles/mc3d_holey_bench.json                        (on the GPU)
    python tools/mc3d_holey_bench.py --reference-out profiles/mc3d_holey_reference_cpu.json      (on a CPU, with the reference)

Cases, 4 096 levels each, for both problems at 7^3 and at 15^3:
  random       tiles drawn independently (tests/mc3d_holey_levels.py random_set), a random valid pair of holes: almost never
               connected, many AIR regions, short searches
  structured   terrains between holes levelled to them (structured_set): steps, cliffs, pits to jump, ceilings, items on the
               ground, in mid-air and buried; more than half connect
Per case the tool times `calls` evaluate() calls between two device synchronisations with the host clock, `windows` times, after
a warm-up of every case; the kernel alone is the time between two device events around one pcgrl_mc3d_holey_evaluate call on
prepared buffers (no allocation, no other kernel), averaged over `calls` calls.  The accepted pops come from the kernel's own
`play` record; the critical level is the one with the most accepted pops (both searches of a dungeon run side by side, so the
larger of the two counts), and kernel time / its pops / the levels a workgroup strides over bounds the time per pop from
above.  The first levels of each case are checked against tests/mc3d_holey_rules.py, which is timed on them on one host core.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import mc3d_holey_levels as Lv  # noqa: E402
import mc3d_holey_rules as R  # noqa: E402

N = 4096
SHAPES = [(7, 7, 7), (15, 15, 15)]
REFERENCE_FILE = os.path.join(ROOT, "profiles", "mc3d_holey_reference_cpu.json")


def case_levels(problem, shape, kind, n=N):
    seed = 9100 + 10 * shape[0] + (1 if problem == "maze" else 0)
    return Lv.random_set(problem, shape, n, seed) if kind == "random" else Lv.structured_set(problem, shape, n, seed + 5)


def cases():
    return [(p, s, k) for p in ("dungeon", "maze") for s in SHAPES for k in ("random", "structured")]


def key(problem, shape, kind):
    return "%s-%dx%dx%d-%s" % ((problem,) + tuple(shape) + (kind,))


def reference_cpu(levels, out):
    """the reference's own get_stats on the first `levels` levels of every case, one host core"""
    import gen_golden_mc3d_holey as G
    import ref_env
    assert ref_env.available(), "this mode needs the reference tree"
    res = {"method": "time.perf_counter around get_stats of an instance made with __new__ (the maze is called twice per map and "
                     "one call's share is reported), the bordered string map built outside the clock; one host core",
           "levels": levels, "cases": {}}
    for problem, shape, kind in cases():
        grids, holes = case_levels(problem, shape, kind, levels)
        G.reference_level(problem, grids[0], holes[0])  # the imports and the first call stay outside the clock
        # the recorder's function, timed whole, then the map building subtracted
        t0 = time.perf_counter()
        for i in range(levels):
            R.bordered_map(grids[i], holes[i])
        build = time.perf_counter() - t0
        t0 = time.perf_counter()
        for i in range(levels):
            G.reference_level(problem, grids[i], holes[i])
        total = time.perf_counter() - t0
        per = max(0.0, total - build) / levels / (2 if problem == "maze" else 1)
        res["cases"][key(problem, shape, kind)] = {"seconds_per_get_stats": per}
        print(key(problem, shape, kind), "%.2f ms" % (per * 1e3), flush=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


def gpu(calls, windows, rules_levels):
    import torch
    from control_pcgrl_amd import Mc3dHoleyEvaluator, _lib
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = "cuda:0"
    L = _lib.lib()
    reference = json.load(open(REFERENCE_FILE))["cases"] if os.path.exists(REFERENCE_FILE) else {}
    out = {}
    for problem, shape, kind in cases():
        name = key(problem, shape, kind)
        grids, holes = case_levels(problem, shape, kind)
        ev = Mc3dHoleyEvaluator(problem, shape, dev)
        g, h = torch.from_numpy(grids).to(dev), torch.from_numpy(holes).to(dev)
        got = ev.evaluate(g, h, route_cap=64)
        t0 = time.perf_counter()
        want = [R.evaluate(problem, grids[i], holes[i]) for i in range(rules_levels)]
        rules_s = (time.perf_counter() - t0) / rules_levels
        for i, w in enumerate(want):
            assert got["stats"][i].tolist() == w["stats"] and got["play"][i].tolist() == w["play"], (name, i)
            assert int(got["route_len"][i]) == len(w["route"]), (name, i)
        play, stats = got["play"].cpu().numpy(), got["stats"].cpu().numpy()
        pops = play[:, 1] + play[:, 3]
        critical = np.maximum(play[:, 1], play[:, 3])
        connected = (stats[:, 2] > 0) if problem == "maze" else (got["leg_len"].cpu().numpy() > 0).all(1)
        for _ in range(2):
            ev.evaluate(g, h)
        torch.cuda.synchronize()
        ms = []
        for _ in range(windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                ev.evaluate(g, h)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / calls * 1e3)
        st = torch.empty((N, len(ev.stat_keys)), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kernel = []
        for _ in range(calls):
            start.record()
            _lib.check(L.pcgrl_mc3d_holey_evaluate(C.byref(ev._cfg), N, g.data_ptr(), h.data_ptr(), ev._workspace.data_ptr(),
                                                   ev._workspace_bytes, 0, st.data_ptr(), *([None] * 11), stream))
            end.record()
            torch.cuda.synchronize()
            kernel.append(start.elapsed_time(end))
        ev.check_errors()
        strides = -(-N // min(N, ev.max_blocks))
        k_ms = float(np.mean(kernel))
        r = {"connected_fraction": float(connected.mean()), "regions_mean": float(stats[:, 0].mean()),
             "accepted_pops": {"mean": float(pops.mean()), "max": int(pops.max()), "critical_level": int(critical.max())},
             "ms_per_call": {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))},
             "kernel_ms": {"mean": k_ms, "min": float(np.min(kernel)), "max": float(np.max(kernel))},
             "levels_per_s": N / (float(np.mean(ms)) * 1e-3), "workgroups": min(N, ev.max_blocks), "levels_per_workgroup": strides,
             "workspace_bytes": ev._workspace_bytes,
             "us_per_pop_critical_level_upper_bound": k_ms * 1e3 / max(1, int(critical.max())) / strides,
             "rules": {"levels": rules_levels, "seconds_per_level": rules_s,
                       "us_per_accepted_pop": rules_s * rules_levels * 1e6 / max(1, int(pops[:rules_levels].sum()))}}
        r["speedup_over_rules_one_core"] = rules_s * r["levels_per_s"]
        if name in reference:
            r["reference_get_stats_seconds"] = reference[name]["seconds_per_get_stats"]
            r["speedup_over_reference_one_core"] = reference[name]["seconds_per_get_stats"] * r["levels_per_s"]
        else:
            r["reference_get_stats_seconds"] = "not measured"
        out[name] = r
        print(name, json.dumps(r), flush=True)
        ev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--rules-levels", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference-out", default=None)
    ap.add_argument("--reference-levels", type=int, default=12)
    a = ap.parse_args()
    if a.reference_out:
        reference_cpu(a.reference_levels, a.reference_out)
        return
    res = {"method": "host clock around --calls evaluate() calls between device synchronisations, --windows windows per case "
                     "after a warm-up; kernel_ms: device events around one pcgrl_mc3d_holey_evaluate call; rules on one host "
                     "core over --rules-levels levels per case in the same run; the reference's get_stats from "
                     "profiles/mc3d_holey_reference_cpu.json (another machine's CPU: a context figure, not a same-run ratio)",
           "levels": N, "calls": a.calls, "windows": a.windows,
           "mapping": "one workgroup of two waves per level, a search on lane 0 of a wave"}
    res["cases"] = gpu(a.calls, a.windows, a.rules_levels)
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
