#!/usr/bin/env python3
"""Time per call of SmbVecEnv.export_state, a full load_state_dict(blob) and a masked one of every 16th env, on stock-size
(16 x 116) Mario envs, beside torch.Tensor.clone() of a uint8 tensor of state_bytes in the same run.

    python tools/smb_state_bench.py [--envs 4096] [--calls 200] [--windows 5] [--warmup 20] [--out profiles/smb_state_bench.json]

A window is `--calls` calls of one kind on one stream between two HIP events, after `--warmup` calls; the kinds alternate and the
cycle repeats `--windows` times.  The figure of a kind is the mean over its windows of (event time / calls); the windows' minimum
and maximum are kept beside it.  An import waits for the stream once per call to check the header on the host, so its figure is
a host-paced one -- what a caller pays; the import kernel alone is not timed.  `copy_into` is the plain copy without clone()'s
allocation.  An eager window of calls this short is paced by the host's enqueue rate as much as by the device, so the kinds that
can be captured (clone, copy_into, export_state) are also timed as ONE HIP graph of `--calls` calls on one stream, replayed
between two events: `graph_us_per_call`, the device's own pace.  The calls are off the stepping path: no ratio is demanded, the
multiple of the plain copy is reported."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from control_pcgrl_amd import SmbVecEnv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "smb_state_bench needs the GPU: a host run gives no time"
assert args.calls >= 100, "at least 100 calls a window"

H, W, DEV = 16, 116, "cuda:0"
n = args.envs
# the state calls never search: a small solver_power keeps the workspace, which no call here touches, small
env = SmbVecEnv("turtle", (H, W), n, device=DEV, solver_power=300, seeds=np.arange(n))
env.reset()
g = torch.Generator().manual_seed(0)
for _ in range(10):
    env.step(torch.randint(0, env.num_actions, (n,), generator=g, dtype=torch.int32).to(DEV))
nbytes = env.state_bytes
image = env.export_state()
out = torch.empty_like(image)
plain = torch.empty(nbytes, dtype=torch.uint8, device=DEV).copy_(image)
every16 = torch.zeros(n, dtype=torch.uint8, device=DEV)
every16[::16] = 1
sd = {"blob": image}
KINDS = {
    "clone": lambda: plain.clone(),
    "copy_into": lambda: out.copy_(plain),  # the plain copy without clone()'s allocation
    "export_state": lambda: env.export_state(out),
    "import_full": lambda: env.load_state_dict(sd),
    "import_every_16th": lambda: env.load_state_dict(sd, mask=every16),
}
times = {k: [] for k in KINDS}
for w in range(args.windows):
    for k, fn in KINDS.items():
        for _ in range(args.warmup):
            fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.calls):
            fn()
        stop.record()
        torch.cuda.synchronize()
        times[k].append(start.elapsed_time(stop) * 1e3 / args.calls)
assert torch.equal(env.export_state(), image)  # the imports put back what the export took

# the capturable kinds as one graph of --calls calls: no host pacing between the calls
graph_times = {}
side = torch.cuda.Stream()
for k in ("clone", "copy_into", "export_state"):
    fn = KINDS[k]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kept = [fn() for _ in range(args.calls)]  # (clone's results stay alive, as a caller's would)
    graph.replay()
    graph_times[k] = []
    for w in range(args.windows):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        graph.replay()
        stop.record()
        torch.cuda.synchronize()
        graph_times[k].append(start.elapsed_time(stop) * 1e3 / args.calls)
    del kept, graph
assert torch.equal(out, image)
env.check_errors()

result = {"method": "HIP events around --calls calls of one kind on one stream after --warmup calls; kinds alternate, windows "
                    "repeated in one process; microseconds per call, mean / min / max over the windows.  The imports wait "
                    "for the stream once per call (the header check on the host), so theirs is a host-paced figure",
          "envs": n, "map_shape": [H, W], "state_bytes": nbytes, "bytes_per_env": (nbytes - 256) // n, "calls": args.calls,
          "warmup": args.warmup, "windows": args.windows, "device": torch.cuda.get_device_name(0), "us_per_call": {}}
for k, v in times.items():
    result["us_per_call"][k] = {"mean": statistics.mean(v), "min": min(v), "max": max(v)}
clone = result["us_per_call"]["clone"]["mean"]
result["multiple_of_clone"] = {k: result["us_per_call"][k]["mean"] / clone for k in KINDS if k != "clone"}
result["graph_us_per_call"] = {k: {"mean": statistics.mean(v), "min": min(v), "max": max(v)} for k, v in graph_times.items()}
gclone = result["graph_us_per_call"]["clone"]["mean"]
result["graph_multiple_of_clone"] = {k: result["graph_us_per_call"][k]["mean"] / gclone for k in graph_times if k != "clone"}
# read + write of the image's bytes over the graph's time per call: what the copy achieves, not a share of a kernel's peak
result["export_gb_per_s"] = 2 * nbytes / (result["graph_us_per_call"]["export_state"]["mean"] * 1e-6) / 1e9
result["clone_gb_per_s"] = 2 * nbytes / (gclone * 1e-6) / 1e9
line = json.dumps(result, indent=1)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
env.close()
