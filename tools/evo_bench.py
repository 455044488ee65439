"""Times the pieces of NCA evolution on one MI355X -> profiles/evo_bench.json.

    python tools/evo_bench.py [--out profiles/evo_bench.json] [--reps 9] [--time-limit 300]

  ask_genomes  4096 children at P = 1730 and 3656 from a [100, 100] archive with 4096 occupied cells, against
               parents[idx] + torch.randn_like(...) * sigma on the same device in the same run.  Only the time is compared: the
               two streams differ.
  aggregate    G = 4096, S = 10, D = 2 against torch's mean / std / sum of the same tensors.
  generation   Lode Runner stock 8 x 12, 1024 genomes x 10 seeds: one NcaEvolution.generation(), uncaptured and as one captured
               graph, and each stage alone.

One process; it ends itself after --time-limit seconds.  Times are medians of --reps calls after a warm-up, device events around
the call (the uncaptured generation also has its host wall time: the enqueue is part of it).
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from control_pcgrl_amd import (GenomeArchive, LodeRunnerEvaluator, NcaEvolution, evaluator_score, evo, generator_for,  # noqa: E402
                               genome_archive_for, nca)

DEV = "cuda:0"
HBM_PEAK = 8.0e12  # bytes/s
FP64_NO_FMA = 39.3e12  # float64 vector operations/s without fused multiply-add (half of 78.6 TFLOP/s)


def timed(fn, reps, wall=False):
    fn()
    torch.cuda.synchronize()
    times, walls = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        walls.append(time.perf_counter() - t0)
        times.append(a.elapsed_time(b) * 1e-3)
    return (float(np.median(times)), float(np.median(walls))) if wall else float(np.median(times))


def bench_ask(P, n, reps):
    rng = np.random.default_rng(P)
    arc = GenomeArchive((100, 100), [(0.0, 1.0), (0.0, 1.0)], P, device=DEV)
    k = 4096
    cells = torch.as_tensor(rng.permutation(10000)[:k].astype(np.int32)).to(DEV)
    rows = torch.as_tensor((rng.standard_normal((k, P)) * 0.2).astype(np.float32)).to(DEV)
    arc.add(rows, torch.as_tensor(rng.random(k)).to(DEV), cells=cells)
    out = (torch.empty((n, P), dtype=torch.float32, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV))
    sigma = 0.1
    t_ask = timed(lambda: arc.ask(n, seed=1, sigma=sigma, out=out), reps)
    arc.check_errors()
    kids = out[0]
    var = ((kids - arc.dense().genomes[out[1].long()]) / sigma).var().item()
    idx = torch.randint(0, k, (n,), device=DEV)

    def torch_side():
        p = rows[idx]
        return p + torch.randn_like(p) * sigma

    t_torch = timed(torch_side, reps)
    arc.close()
    byts = 2 * n * P * 4
    return {"case": f"ask_genomes P={P}", "n": n, "n_params": P, "kernel_s": t_ask, "torch_s": t_torch,
            "torch_over_kernel": t_torch / t_ask, "bytes": byts, "bytes_per_s": byts / t_ask,
            "share_of_hbm_peak": byts / t_ask / HBM_PEAK, "elements_per_s": n * P / t_ask,
            "variance_of_the_draws": var}


def bench_aggregate(G, S, D, reps):
    rng = np.random.default_rng(0)
    obj = torch.as_tensor(rng.standard_normal((G, S))).to(DEV)
    beh = torch.as_tensor(rng.random((G, S, D))).to(DEV)
    ns = torch.as_tensor(rng.integers(0, 10, (G, S)).astype(np.int32)).to(DEV)
    out = evo.aggregate(obj, beh, ns)
    t_k = timed(lambda: evo.aggregate(obj, beh, ns, out=out), reps)

    def torch_side():
        return (beh.mean(dim=1), (10.0 * obj.sum(dim=1)) / S, -ns.sum(dim=1), -beh.std(dim=1, unbiased=False).sum(dim=1) / D,
                (ns >= 0).all(dim=1))

    t_t = timed(torch_side, reps)
    return {"case": f"aggregate G={G} S={S} D={D}", "kernel_s": t_k, "torch_s": t_t, "torch_over_kernel": t_t / t_k}


def bench_generation(G, S, reps):
    ev = LodeRunnerEvaluator((8, 12), device=DEV)
    names = ["emptiness", "path-length"]
    arc = genome_archive_for(ev, names)
    gen = generator_for(ev, n_steps=10)
    score = evaluator_score(ev, names, gold_cap=0)
    evolution = NcaEvolution(gen, score, arc)
    rng = np.random.default_rng(5)
    T = ev.spec.n_tiles
    init = torch.as_tensor(rng.integers(0, T, (S, 8, 12), dtype=np.uint8)).to(DEV)
    mean = torch.as_tensor((rng.standard_normal(arc.n_params) * 0.3).astype(np.float32)).to(DEV)
    evolution.generation(init, G, seed=1, sigma=0.3, first=True, mean=mean)
    t_dev, t_wall = timed(lambda: evolution.generation(init, G, seed=1, sigma=0.1), reps, wall=True)
    res = evolution.generation(init, G, seed=1, sigma=0.1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        evolution.generation(init, G, seed=1, sigma=0.1)
    t_graph, t_graph_wall = timed(graph.replay, reps, wall=True)
    # each stage alone, on the tensors of the last generation
    levels = res.levels.view(G * S, 8, 12)
    objective, behaviours = score(levels)
    stages = {
        "ask": timed(lambda: arc.ask(G, seed=1, sigma=0.1, out=(res.genomes, res.parent_cell)), reps),
        "generate": timed(lambda: gen.generate(res.genomes, init, out=evolution._buffers(G, S).gen), reps),
        "evaluate": timed(lambda: ev.evaluate(levels, gold_cap=0), reps),
        "behaviour": timed(lambda: ev.behaviour(levels, names), reps),
        "aggregate": timed(lambda: evo.aggregate(objective.reshape(G, S), behaviours.reshape(G, S, -1), res.n_step,
                                                 out=res.aggregate), reps),
        "diversity": timed(lambda: ev.diversity(levels, group=S), reps),
        "add": timed(lambda: arc.add(res.genomes, res.aggregate.objective, res.aggregate.behaviours), reps),
    }
    total = sum(stages.values())
    arc.check_errors()
    row = {"case": f"generation loderunner 8x12 G={G} S={S}", "uncaptured_device_s": t_dev, "uncaptured_wall_s": t_wall,
           "captured_device_s": t_graph, "captured_wall_s": t_graph_wall, "stages_s": stages,
           "stage_share": {k: v / total for k, v in stages.items()}, "occupied": arc.stats().count,
           "n_params": nca.n_params(T)}
    arc.close(), gen.close(), ev.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evo_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--time-limit", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.time_limit)  # the process ends itself
    rows = []
    for P in (1730, 3656):
        rows.append(bench_ask(P, 4096, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    rows.append(bench_aggregate(4096, 10, 2, args.reps))
    print(json.dumps(rows[-1]), flush=True)
    rows.append(bench_generation(1024, 10, args.reps))
    print(json.dumps(rows[-1]), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hbm_peak_bytes_per_s": HBM_PEAK,
              "fp64_vector_ops_per_s_without_fma": FP64_NO_FMA, "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
