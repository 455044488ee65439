#!/usr/bin/env python3
"""bench.py -- env-steps/s of the PCGRL hot path on MI355X (BASELINE.json metric).

A "step" is one pcgrl_step launch: every env of the rank's batch takes one action (representation update ->
stats -> reward -> done/auto-reset -> cropped one-hot observation written to HBM).  Workload at N=1 is
BASELINE configs[1]: binary-narrow 16x16, 4096 envs on one GPU, uniform random actions, auto-reset.
Inputs (actions) are resident in HBM before the timed region; outputs (obs/reward/done/stats) are written to HBM.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]

--dump-outputs DIR: the outputs of the last timed step as DIR/<name>.npy (float32 / float64).  Inputs are seeded (env seeds,
action pools, injected maps), so two builds run with the same arguments can be compared output for output.

N > 1: one process per GPU.  Started by `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`
the script is one rank (RANK / LOCAL_RANK / WORLD_SIZE from the environment); started plainly it launches the N
ranks itself (child processes, before anything in this process touches the GPU) and relays rank 0's line.

Timed region (every N) = K launches + the pcgrl_reduce_episodes launch + ONE synchronise, bracketed by barrier +
synchronize, max over ranks.  N > 1: the path's only collective -- the RCCL all-gather of the episode sums + its
device->host copy -- ships the PREVIOUS interval's sums on a side stream while this interval steps (SURVEY 8 e), so the
N > 1 region has the N = 1 region's structure and no rank waits for another inside it (--exchange serial: round 5's form).
A rank that does not finish within PCGRL_BENCH_RANK_TIMEOUT seconds (default 1500) exits with code 3.

Prints ONE JSON line (rank 0).  `roofline` prices the step kernel against HBM bandwidth with the algorithmic
bytes of SURVEY.md section 8(d): `achieved` / `frac` use the same wall clock as `value`, `achieved_hip_events` /
`frac_hip_events` the HIP-event time of the K launches on the launch stream.  `cpu_baseline` is the CPU oracle
(oracle/, a port of the reference's algorithm) timed on this box's host cores on a bounded sample of the same workload.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# algorithmic bytes per env-step (action in + grid read/1 B write + uint8 one-hot obs out +
# reward/done/stats/pos out)
ALGO_BYTES = {"binary-narrow": 4 + 257 + 32 * 32 * 3 + (4 + 1 + 8 + 2),
              "zelda-turtle": 4 + 257 + 32 * 32 * 9 + (4 + 1 + 28 + 2),
              "sokoban-wide": 4 + 257 + 16 * 16 * 5 + (4 + 1 + 28 + 0),
              "minecraft_3D_maze-narrow": 4 + 344 + 14 ** 3 * 4 + (4 + 1 + 12 + 3),
              # SURVEY 8(f) N2 representation wrappers: + static mask read and one more obs channel / 9 action entries
              "binary-narrow-static": 4 + 257 + 32 + 32 * 32 * 4 + (4 + 1 + 8 + 2),
              "binary-narrow-patch3x3": 36 + 257 + 32 * 32 * 3 + (4 + 1 + 8 + 2),
              # SURVEY 8(d) "BFS-active" variant: maps with exactly one player / key / door, actions restricted to moves
              # and {empty, solid, enemy} placements, so both single-source searches run on every change
              "zelda-turtle-bfs": 4 + 257 + 32 * 32 * 9 + (4 + 1 + 28 + 2),
              # "solver-active" sokoban: playable levels (one player, k crates / targets, one region) so that the device
              # solver (engine.py BFS / A* cascade) runs inside the step launches
              "sokoban-wide-solver": 4 + 257 + 16 * 16 * 5 + (4 + 1 + 28 + 0),
              # the reference's stock task configs off the 16x16 point: configs/task/binary_big.yaml:5-6,
              # binary_bigger.yaml:5-6, zelda_big.yaml:5-6, configs/config.py:153-157 (MinecraftConfig 15^3, crop 30^3);
              # same formula: action + map read / 1 B write + uint8 one-hot window + reward / done / stats / pos
              "binary_big-narrow": 4 + (32 * 32 + 1) + 64 * 64 * 3 + (4 + 1 + 8 + 2),
              "binary_bigger-narrow": 4 + (64 * 64 + 1) + 128 * 128 * 3 + (4 + 1 + 8 + 2),
              "zelda_big-turtle": 4 + (32 * 32 + 1) + 64 * 64 * 9 + (4 + 1 + 28 + 2),
              "zelda_bigger-turtle": 4 + (64 * 64 + 1) + 128 * 128 * 9 + (4 + 1 + 28 + 2),  # configs/task/zelda_bigger.yaml:5-6
              "minecraft_3D_maze-narrow-15": 4 + (15 ** 3 + 1) + 30 ** 3 * 4 + (4 + 1 + 12 + 3),
              # evolution driver's call pattern (evo/evolve.py:1083-1120): n_cells x rep.update (+ observation), then one
              # get_stats; per update: action + map read / 1 B write + observation + pos; the statistics pass adds
              # (map read + stats) once per n_cells updates
              "binary-narrow-evo": 4 + 257 + 32 * 32 * 3 + 2 + (256 + 8) / 256,
              # Problem.get_stats on caller maps (pcgrl_stats_for_grids): map read + the statistics
              "binary-stats-for-grids": 256 + 8,
              "zelda-stats-for-grids": 256 + 28}
# BASELINE.json configs: (problem, representation, map_shape, envs per GPU)
WORKLOADS = {"binary-narrow": ("binary", "narrow", (16, 16), 4096), "zelda-turtle": ("zelda", "turtle", (16, 16), 4096),
             "sokoban-wide": ("sokoban", "wide", (16, 16), 2048),
             "minecraft_3D_maze-narrow": ("minecraft_3D_maze", "narrow", (7, 7, 7), 1024),
             "binary-narrow-static": ("binary", "narrow", (16, 16), 4096, dict(static_prob=0.3, n_static_walls=3)),
             "binary-narrow-patch3x3": ("binary", "narrow", (16, 16), 4096, dict(act_window=[3, 3])),
             "zelda-turtle-bfs": ("zelda", "turtle", (16, 16), 4096),
             "sokoban-wide-solver": ("sokoban", "wide", (16, 16), 2048),
             "binary_big-narrow": ("binary", "narrow", (32, 32), 4096), "binary_bigger-narrow": ("binary", "narrow", (64, 64), 4096),
             "zelda_big-turtle": ("zelda", "turtle", (32, 32), 4096), "zelda_bigger-turtle": ("zelda", "turtle", (64, 64), 4096),
             "minecraft_3D_maze-narrow-15": ("minecraft_3D_maze", "narrow", (15, 15, 15), 1024),
             "binary-narrow-evo": ("binary", "narrow", (16, 16), 4096),
             "binary-stats-for-grids": ("binary", "narrow", (16, 16), 65536),
             "zelda-stats-for-grids": ("zelda", "narrow", (16, 16), 65536)}
BFS_ACTIONS = [0, 1, 2, 3, 4 + 0, 4 + 1, 4 + 5, 4 + 6, 4 + 7]  # turtle moves, then empty / solid / bat / scorpion / spider


def bfs_active_maps(n, seed):
    """zelda maps with exactly one player (2), key (3) and door (4) among empty / solid / enemy tiles"""
    import numpy as np
    rng = np.random.default_rng(seed)
    g = rng.choice(np.array([0, 1, 5, 6, 7], np.uint8), size=(n, 256), p=[0.62, 0.26, 0.04, 0.04, 0.04])
    for i in range(n):
        c = rng.choice(256, size=3, replace=False)
        g[i, c[0]], g[i, c[1]], g[i, c[2]] = 2, 3, 4
    return g.reshape(n, 16, 16)

def solver_active_maps(n, seed):
    """sokoban maps that meet the solver's precondition (sokoban_prob.py:172-177): one small room carved into solid with
    one player and k crates / k targets; plus, per env, the cells an edit may touch without (usually) splitting the room:
    the room and its 4-neighbourhood.  Returns (maps uint8 [n,16,16], cells: list of int arrays in the wide action's
    column-major cell index)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    g = np.ones((n, 16, 16), np.uint8)
    cells = []
    for i in range(n):
        h, w = int(rng.integers(3, 6)), int(rng.integers(3, 7))
        y0, x0 = int(rng.integers(1, 16 - h)), int(rng.integers(1, 16 - w))
        g[i, y0:y0 + h, x0:x0 + w] = 0
        k = int(rng.integers(1, 4))
        pick = rng.permutation(h * w)[:1 + 2 * k]
        for c, t in zip(pick, [2] + [3] * k + [4] * k):
            g[i, y0 + c // w, x0 + c % w] = t
        m = np.zeros((16, 16), bool)
        m[y0:y0 + h, x0 - 1:x0 + w + 1] = True
        m[y0 - 1:y0 + h + 1, x0:x0 + w] = True
        r, c = np.nonzero(m)
        cells.append((c * 16 + r).astype(np.int32))  # wide_rep.py:40-45: x = row, y = column
    return g, cells


def solver_active_actions(cells, pool, seed):
    """int32 [pool, n]: floor or wall (never a player / crate / target) on one of the env's candidate cells"""
    import numpy as np
    rng = np.random.default_rng(seed)
    a = np.empty((pool, len(cells)), np.int32)
    for i, c in enumerate(cells):
        a[:, i] = c[rng.integers(0, len(c), pool)] * 5 + rng.integers(0, 2, pool)
    return a


HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
DUMP_LIMIT_BYTES = 64_000_000  # --dump-outputs: all files of one run together (data + .npy headers)
DUMP_SAMPLE_SEED = 20240521    # --dump-outputs: which envs go into the files when not all of them fit


def dump_outputs(out_dir, per_env, shared, rank, world):
    """--dump-outputs: write what the timed path handed its caller in its last step as <out_dir>/<name>.npy.

    `per_env`: name -> (device tensor with the env index as its first axis, numpy dtype float32 / float64); `shared`: name ->
    host array that is not per env (written by rank 0 only).  When the per-env arrays of all envs exceed this rank's share of
    DUMP_LIMIT_BYTES, a fixed, seeded sample of envs (the same envs in every array, in ascending order) is written instead;
    `env_sample` then holds their indices.  With N > 1 ranks every rank writes its own shard as <name>.rank<r>.npy."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    suffix = f".rank{rank}" if world > 1 else ""
    header = 128  # bytes of one .npy header (numpy pads the header to a multiple of 64; short shapes fit 128)
    budget = DUMP_LIMIT_BYTES // world - header * (len(per_env) + 1)
    if rank == 0:
        budget -= sum(header + np.asarray(a).size * 8 for a in shared.values())
    n = next(iter(per_env.values()))[0].shape[0]
    row_bytes = sum(t[0].numel() * np.dtype(dt).itemsize for t, dt in per_env.values())
    idx = None
    if n * row_bytes > budget:
        m = max(1, budget // (row_bytes + 8))  # (+ the float64 index of each sampled env)
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, size=m, replace=False))
        np.save(os.path.join(out_dir, f"env_sample{suffix}.npy"), idx.astype(np.float64))
    written = []
    for name, (t, dt) in per_env.items():
        if idx is not None:
            t = t.index_select(0, torch.as_tensor(idx, device=t.device))
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), t.cpu().numpy().astype(dt))
        written.append(name)
    if rank == 0:
        for name, a in shared.items():
            np.save(os.path.join(out_dir, f"{name}.npy"), np.asarray(a, dtype=np.float64))
            written.append(name)
    return {"dir": out_dir, "arrays": written, "envs": n if idx is None else int(len(idx)), "of_envs": n}


def main():
    # (multi-process GPU work on this pool: the host driver only supports dmabuf IPC; RCCL needs it before HIP starts)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=-1, help="timed launches (default 20000; fewer for the big-map workloads)")
    ap.add_argument("--warmup", type=int, default=-1, help="untimed launches before them (default steps / 10)")
    ap.add_argument("--envs", type=int, default=0, help="envs per GPU (default: the BASELINE.json config's)")
    ap.add_argument("--workload", default="binary-narrow", choices=sorted(ALGO_BYTES))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--graph-steps", type=int, default=-1,
                    help="launch the step kernel through a captured HIP graph of this many steps (0 = eager launches; default: "
                         "125 when --steps >= 250, else eager -- the eager Python loop is host-bound below ~6.3 us per launch)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target wall time of the CPU baseline sample")
    ap.add_argument("--rollout-steps", type=int, default=64,
                    help="also time the open-loop rollout kernel (pcgrl_rollout) with this many steps per launch and "
                         "report it as `open_loop_rollout`; 0 = skip")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / rendezvous / sharding only (gloo, no GPU, nothing timed): what the CPU test of the N > 1 path runs")
    ap.add_argument("--rllib-adapter", type=int, default=-1,
                    help="1 / 0: time PcgrlVectorEnv.vector_step (the RLlib VectorEnv call shape, host arrays out) as the secondary "
                         "object `rllib_adapter`; default: on for the headline workload")
    ap.add_argument("--rollout-launches", type=int, default=200, help="timed pcgrl_rollout launches of the secondary figure")
    ap.add_argument("--force-collective", action="store_true",
                    help="with --gpus 1: initialise a world-size-1 'nccl' (RCCL) process group and close the timed region through the "
                         "N > 1 exchange (device all-gather + device->host copy), so that a 1-GPU box executes the multi-GPU code path")
    ap.add_argument("--closed-loop-steps", type=int, default=-1,
                    help="steps of the secondary figure `closed_loop_device_actions` (a HIP graph of [pcgrl_sample_actions -> pcgrl_step] "
                         "pairs: an action drawn on the device at every step, SURVEY 8(d)'s literal protocol); 0 = skip; default max(steps, 2000)")
    ap.add_argument("--short-protocol", default="fused", choices=["fused", "one", "gcd"],
                    help="runs of 2..125 steps (the driver's --steps 20 --warmup 5): 'fused' = ONE HIP graph of the K step launches + the "
                         "closing pcgrl_reduce_episodes launch, uploaded ahead of time, the W warm-up steps eager; 'one' = round 4's (the "
                         "reduction launched separately); 'gcd' = a graph of gcd(W, K) steps, W / G untimed + K / G timed replays")
    ap.add_argument("--sub-batches", default="2,4",
                    help="secondary figure `async_sub_batches`: the batch as k engines of N / k envs on k streams, their step chains captured "
                         "as parallel branches of one HIP graph (SubBatchedVecEnv); comma-separated k values, '' = skip")
    ap.add_argument("--exchange", default="overlap", choices=["overlap", "serial"],
                    help="N > 1 (or --force-collective): 'overlap' (default) = the timed region has the N = 1 region's structure -- K step "
                         "launches + the pcgrl_reduce_episodes launch + one synchronise -- while the all-gather + device->host copy of the "
                         "PREVIOUS interval's sums run on a side stream under the stepping (SURVEY 8 e: 'issue it on a side stream so it never "
                         "blocks stepping'); 'serial' = round 5's region: reduction -> all-gather -> copy behind the K launches, as the closing barrier")
    ap.add_argument("--solver-budget", type=int, default=0,
                    help="sokoban-wide-solver: asynchronous stepping (pcgrl_set_solver_budget / pcgrl_step_ready) with this many solver "
                         "iteration units per env and launch; `value` then counts the transitions the launches EMITTED (busy envs do not "
                         "step); 0 = synchronous pcgrl_step")
    ap.add_argument("--solver-forms", type=int, default=0,
                    help="sokoban-wide-solver: also time this many steps of the same workload through pcgrl_rollout (8 steps per launch "
                         "between re-injections) and through sub_batches = 4 (secondary object `solver_active_forms`); 0 = skip")
    ap.add_argument("--no-pin", action="store_true", help="do not pin each rank to its own slice of the host cores")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the timed path handed its caller in its last step (obs, reward, done, "
                         "stats; status with --solver-budget; stats only for the stats-for-grids workloads; obs, and stats when a "
                         "refresh ran, for -evo) plus the timed region's episode sums as DIR/<name>.npy in float32 / float64, "
                         f"at most {DUMP_LIMIT_BYTES // 10**6} MB in all (a fixed, seeded sample of envs when all of them do not fit)")
    args = ap.parse_args()
    if args.steps == 0:
        ap.error("--steps must be at least 1 (or negative for the default)")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world == 1 and "RANK" not in os.environ:
        # plain `python bench.py --gpus N`: this process becomes the launcher.  It never loads a GPU runtime (the device count
        # comes from the kernel driver's topology files), and the ranks are ordinary child processes -- never an exec of a
        # process that holds a GPU.
        if not args.dry_run and not os.environ.get("PCGRL_BENCH_SINGLE_DEVICE"):
            have = gpus_without_runtime()
            if have is not None and args.gpus > have:
                sys.exit(f"bench.py: --gpus {args.gpus} but this node shows {have} GPU(s): one rank per GPU, nothing was started")
        sys.exit(launch_ranks(args.gpus))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: start it plainly (it launches its own ranks) "
                 f"or under torch.distributed.run with --nproc-per-node {args.gpus}")

    # N > 1: every rank keeps to its own slice of the host cores (launch threads, the runtime's helpers and RCCL's proxy do not
    # migrate onto another rank's cores); set before anything touches the GPU.  Rank 0 widens its mask again for `cpu_baseline`.
    all_cores = None
    pinned = None
    try:
        all_cores = sorted(os.sched_getaffinity(0))
        lw = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
        lr = int(os.environ.get("LOCAL_RANK", "0"))
        if world > 1 and not args.no_pin and lw > 1 and len(all_cores) >= 2 * lw:
            per = len(all_cores) // lw
            pinned = all_cores[lr * per:(lr + 1) * per]
            os.sched_setaffinity(0, pinned)
    except (AttributeError, OSError):
        pinned = None

    import numpy as np
    import torch
    import torch.distributed as dist

    from control_pcgrl_amd import VecPcgrlEnv
    from control_pcgrl_amd.dist import shard_env_range, shard_seeds

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # A rank that hangs (a peer that never joins a collective, a wedged device) must END, with a non-zero code -- never a
    # re-exec or an in-process fallback of a process that has touched the GPU: the launcher (ours or torch.distributed.run) then
    # stops the other ranks and the run fails visibly instead of sitting in a collective for ever.
    import threading
    rank_timeout = float(os.environ.get("PCGRL_BENCH_RANK_TIMEOUT", "1500"))
    if os.environ.get("PCGRL_BENCH_TEST_HANG_RANK") == str(rank) and os.environ.get("PCGRL_BENCH_TEST_HANG_TIMEOUT"):
        rank_timeout = float(os.environ["PCGRL_BENCH_TEST_HANG_TIMEOUT"])  # (test hook: only the rank that hangs is in a hurry)

    def _rank_timed_out():
        sys.stderr.write(f"bench.py: rank {rank} did not finish within {rank_timeout:.0f} s (PCGRL_BENCH_RANK_TIMEOUT): exit code 3\n")
        sys.stderr.flush()
        os._exit(3)

    watchdog = threading.Timer(rank_timeout, _rank_timed_out)
    watchdog.daemon = True
    watchdog.start()
    if args.dry_run:
        n_envs = args.envs or WORKLOADS[args.workload][3]
        if os.environ.get("PCGRL_BENCH_TEST_HANG_RANK") == str(rank):  # (test hook: a rank that never reaches the rendezvous)
            time.sleep(1e6)
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo")
        mine = torch.tensor(shard_seeds(0x5EED, n_envs * world, rank, world)[:: max(1, n_envs - 1)], dtype=torch.int64)
        every = [torch.zeros_like(mine) for _ in range(world)]
        if world > 1:
            dist.all_gather(every, mine)
        else:
            every = [mine]
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "envs_per_gpu": n_envs, "global_envs": n_envs * world,
                              "first_last_seed_per_rank": [e.tolist() for e in every]}), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return
    # test hooks (a 1-GPU box can still exercise the multi-process path): all ranks on one device, gloo collectives
    if os.environ.get("PCGRL_BENCH_SINGLE_DEVICE"):
        local_rank = 0
    backend = os.environ.get("PCGRL_BENCH_BACKEND", "nccl")
    if local_rank >= torch.cuda.device_count():
        sys.exit(f"bench.py: rank {rank} wants cuda:{local_rank} but this node shows {torch.cuda.device_count()} GPU(s)")
    torch.cuda.set_device(local_rank)
    dev = torch.device(f"cuda:{local_rank}")
    use_coll = world > 1 or args.force_collective  # the N > 1 exchange path (also with ONE rank under --force-collective)
    if use_coll:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1 and "MASTER_PORT" not in os.environ:
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", str(world))
        import datetime
        pg_timeout = datetime.timedelta(seconds=min(rank_timeout, 600.0))  # (a collective that waits longer than this aborts the rank)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, rank=rank, world_size=world, timeout=pg_timeout)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world, timeout=pg_timeout)
    coll_dev = dev if backend == "nccl" else torch.device("cpu")

    problem, rep, shape, default_envs = WORKLOADS[args.workload][:4]
    wkw = WORKLOADS[args.workload][4] if len(WORKLOADS[args.workload]) > 4 else {}
    N, K, W = (args.envs or default_envs), args.steps, args.warmup
    total_envs = N * world
    solver_active = args.workload == "sokoban-wide-solver"
    bfs_active = args.workload == "zelda-turtle-bfs" or solver_active  # "injected maps" workloads
    evo = args.workload.endswith("-evo")              # K x pcgrl_update (+ obs), one pcgrl_refresh_stats per n_cells updates
    sfg = args.workload.endswith("-stats-for-grids")  # one pcgrl_stats_for_grids_h launch over N caller maps per step
    if args.steps < 0:  # defaults sized so that a plain run finishes within a minute or two whatever the launch costs
        K = args.steps = 2000 if sfg else 20000  # (20 000 launches: >= 1.6 episodes of every workload, 26 of the headline's)
    if args.warmup < 0:
        W = args.warmup = max(K // 10, 5)
    # (stats-for-grids: the maps are the caller's; the engine behind the handle only lends its scratch)
    env = VecPcgrlEnv(problem, rep, shape, 4096 if sfg else N, device=dev, seeds=shard_seeds(0x5EED, total_envs, rank, world)[:4096 if sfg else N],
                      auto_reset=not bfs_active, **wkw)
    inject = None
    budget = args.solver_budget if solver_active else 0
    if solver_active:
        sa_maps, sa_cells = solver_active_maps(N, 77 + rank)
        inject = torch.as_tensor(sa_maps, device=dev).contiguous()
        if budget > 0:  # resumable solver: one workspace per env (synchronous allocation, before anything is timed)
            env.set_solver_budget(budget)
        env.reset(init_grids=inject)
    elif bfs_active:  # no auto-reset: a reset would draw maps with ~10 players, which switch the searches off
        inject = torch.as_tensor(bfs_active_maps(N, 77 + rank), device=dev).contiguous()
        env.reset(init_grids=inject)
    else:
        env.reset()
    if args.dump_outputs:  # (rows the timed path may leave unwritten -- busy envs, update-only steps -- are dumped as zeros)
        for t in (env._reward, env._done, env._stats):
            t.zero_()
    # bfs-active: the turtle eventually overwrites the player / key / door, so the maps are re-injected; solver-active:
    # the edits wear the rooms down (a wall on a crate ends playability), so they come back every few steps
    REINJECT = 8 if solver_active else 128
    # synthetic input: uniform random actions, generated on device before the timed region (seed 1234 + rank)
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    POOL = 1024
    actions = torch.randint(0, env.num_actions, (POOL, N * env.action_entries), generator=g, device=dev, dtype=torch.int32)
    if solver_active:
        actions = torch.as_tensor(solver_active_actions(sa_cells, POOL, 1234 + rank), device=dev).contiguous()
    elif bfs_active:
        actions = torch.tensor(BFS_ACTIONS, dtype=torch.int32, device=dev)[
            torch.randint(0, len(BFS_ACTIONS), (POOL, N), generator=g, device=dev)].contiguous()
    stream = torch.cuda.current_stream(dev)
    sptr = stream.cuda_stream
    base, stride = actions.data_ptr(), N * env.action_entries * 4
    step_raw = env.step_raw
    status_rows = None
    if budget > 0:  # launch k writes its per-env status bytes into row k: the emitted transitions are counted after the clock
        status_rows = torch.zeros((max(K, W, 1), N), dtype=torch.uint8, device=dev)
        st_base = status_rows.data_ptr()

        def step_raw(aptr, strm, _k=[0]):  # noqa: B006  (row = launches issued so far since the last rewind)
            rc = env.step_ready_raw(aptr, st_base + (_k[0] % status_rows.shape[0]) * N, strm)
            _k[0] += 1
            return rc
        step_raw.rewind = lambda: step_raw.__defaults__[0].__setitem__(0, 0)

    EVO_K = int(np.prod(shape))  # evo/evolve.py:2054-2066: N_STEPS = max_changes = n_cells for narrow
    sfg_maps = sfg_out = None
    if sfg:  # maps with a density of their own each (what a population of generators hands to get_stats)
        grng = np.random.default_rng(4242 + rank)
        nt = env.spec.n_tiles
        pr = grng.random((N, nt)) ** 2
        pr /= pr.sum(1, keepdims=True)
        u = grng.random((N, EVO_K))
        sfg_host = (u[:, :, None] >= np.cumsum(pr, 1)[:, None, :]).sum(2).clip(0, nt - 1).astype(np.uint8)
        sfg_maps = torch.as_tensor(sfg_host, device=dev).contiguous()
        sfg_out = torch.empty((N, env.n_stats), dtype=torch.int32, device=dev)

    def run_eager(n, first=0):
        if sfg:
            for k in range(n):
                rc = env._L.pcgrl_stats_for_grids_h(env._h, N, sfg_maps.data_ptr(), sfg_out.data_ptr(), sptr)
                if rc:
                    raise RuntimeError(f"pcgrl_stats_for_grids_h rc={rc}")
            return
        if evo:
            for k in range(first, first + n):
                rc = env._L.pcgrl_update(env._h, base + (k % POOL) * stride, env._ptrs[0], sptr)
                if rc:
                    raise RuntimeError(f"pcgrl_update rc={rc}")
                if (k + 1) % EVO_K == 0:
                    rc = env._L.pcgrl_refresh_stats(env._h, env._ptrs[3], sptr)
                    if rc:
                        raise RuntimeError(f"pcgrl_refresh_stats rc={rc}")
            return
        if inject is None:  # n launches issued by one call into the library (a C host's loop: no per-launch ctypes cost)
            rc = env.step_seq_raw(base, stride // 4, POOL, first % POOL, n, sptr) if n > 0 else 0
            if rc:
                raise RuntimeError(f"pcgrl_step_seq rc={rc}")
            return
        for k in range(first, first + n):
            if inject is not None and k % REINJECT == 0:
                env._L.pcgrl_reset(env._h, None, inject.data_ptr(), None, sptr)
            rc = step_raw(base + (k % POOL) * stride, sptr)
            if rc:
                raise RuntimeError(f"pcgrl_step rc={rc}")

    # The launch-bound inner loop is captured once in a HIP graph of G consecutive steps (each node = one pcgrl_step
    # launch with its own action row) and replayed; K steps = K // G replays + K % G eager launches.  G = 125 is
    # coprime with the narrow scan period (256 cells), so every cell keeps receiving fresh random actions.
    # Short runs (the driver's --steps 20 --warmup 5): one graph of all K steps, uploaded to the device ahead of time
    # (hipGraphUpload: no launch), so that the timed region is a single replay; the W warm-up steps are eager launches.
    # Short runs, second form (round 5): a graph of gcd(W, K) steps replayed W / G times untimed and K / G times timed -- the
    # timed replays are then not the exec's first launch (that first launch costs ~60 us, a third of a 20-step region).
    # Measured (round 5, profiles/r05_bench_lines.json): four replays of a 5-step graph cost MORE than one replay of a 20-step
    # graph that was uploaded but never launched (11.2 vs 7.5 us per step: every replay pays its own launch latency and the
    # device idles between replays), so the default puts the whole timed region into one graph: K steps + the reduction.
    import math
    G_short = K if 2 <= K <= 125 else 0
    if G_short and args.short_protocol == "gcd" and W >= 2 and math.gcd(W, K) >= 2:
        G_short = math.gcd(W, K)
    G = args.graph_steps if args.graph_steps >= 0 else ((125 if K >= 250 else G_short) if inject is None else 0)
    if evo or sfg:
        G = 0
    # the reporting path's buffers (pinned host memory takes milliseconds to allocate: nothing slow may sit between the
    # warm-up steps and the timed region)
    ep_dev = torch.zeros(3 + env.n_stats, dtype=torch.float64, device=dev)
    ep_host = torch.zeros(3 + env.n_stats, dtype=torch.float64).pin_memory()
    done_ev = torch.cuda.Event()
    fuse_reduce = bool(G > 0 and G == K and 2 <= K <= 125 and args.short_protocol == "fused")
    overlap = bool(use_coll and args.exchange == "overlap")
    local_eps = [0.0]  # this rank's own episode count of the last reduction (test evidence)
    ep_all_dev = torch.zeros(world * (3 + env.n_stats), dtype=torch.float64, device=dev)
    ep_all_host = torch.zeros(world * (3 + env.n_stats), dtype=torch.float64).pin_memory()
    # overlapped exchange: the previous interval's sums (this rank's), the side stream they are gathered on, its end marker
    ep_prev_dev = torch.zeros(3 + env.n_stats, dtype=torch.float64, device=dev)
    ep_prev_cpu = torch.zeros(3 + env.n_stats, dtype=torch.float64)
    xstream = torch.cuda.Stream(dev) if overlap else None
    ev_x = torch.cuda.Event(enable_timing=True)
    graph = None
    if G > 0:
        # (thread-local capture mode: with N > 1 ranks the RCCL watchdog thread queries events while this thread captures;
        # if the capture fails all the same, the launches are issued eagerly)
        try:
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream(dev)
            side.wait_stream(stream)
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                    cap = torch.cuda.current_stream(dev).cuda_stream
                    for k in range(G):
                        rc = step_raw(base + (k % POOL) * stride, cap)
                        if rc:
                            raise RuntimeError(f"pcgrl_step (capture) rc={rc}")
                    if fuse_reduce:  # the path's exchange starts with this launch: part of the same graph
                        rc = env._L.pcgrl_reduce_episodes(env._h, ep_dev.data_ptr() if use_coll else ep_host.data_ptr(), 1, cap)
                        if rc:
                            raise RuntimeError(f"pcgrl_reduce_episodes (capture) rc={rc}")
            stream.wait_stream(side)
            try:  # (best effort: the first replay of a graph that was never launched is otherwise slower)
                env._L.pcgrl_graph_upload(graph.raw_cuda_graph_exec(), stream.cuda_stream)
                torch.cuda.synchronize(dev)
            except Exception:  # noqa: BLE001
                pass
        except Exception as exc:  # noqa: BLE001
            print(f"[bench] rank {rank}: graph capture failed ({exc!r}); eager launches", file=sys.stderr, flush=True)
            graph = None
            fuse_reduce = False
            torch.cuda.synchronize(dev)
    if graph is None:
        fuse_reduce = False

    def run(n):
        if graph is None or n < G:
            return run_eager(n)
        if fuse_reduce:  # (n == G == K) the region: the graph of the K steps + the reduction
            graph.replay()
            return
        for _ in range(n // G):
            graph.replay()
        run_eager(n % G, first=G)

    def barrier():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def max_over_ranks(x):
        if world == 1:
            return x, [x]
        t = torch.tensor([x], dtype=torch.float64, device=coll_dev)
        every = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(every, t)
        vals = [float(v.item()) for v in every]
        return max(vals), vals

    # Secondary figure, measured FIRST (it also brings the device to its steady clocks before the short timed region
    # below): the open-loop rollout kernel (pcgrl_rollout, GR steps per launch, every observation written), the engine's
    # counterpart of the reference's random-action profiling loop (profile_env.py:124-142).  Its size does not depend
    # on --steps.  Never `value`.
    GR = args.rollout_steps

    def measure_rollout():
        rollout = None
        if GR > 0 and not wkw and not bfs_active and not evo and not sfg and POOL >= GR:  # (bfs-active needs the periodic map injection)
            R = max(args.rollout_launches, 1)
            obs_r = torch.empty((GR, N) + env.obs_shape, dtype=torch.uint8, device=dev)
            rew_r = torch.empty((GR, N), dtype=torch.float32, device=dev)
            done_r = torch.empty((GR, N), dtype=torch.uint8, device=dev)
            stats_r = torch.empty((GR, N, env.n_stats), dtype=torch.int32, device=dev)

            def run_rollouts(n):
                for i in range(n):
                    rc = env._L.pcgrl_rollout(env._h, base + ((i * GR) % (POOL - GR + 1)) * stride, GR, 1, obs_r.data_ptr(), 0,
                                              rew_r.data_ptr(), done_r.data_ptr(), stats_r.data_ptr(), sptr)
                    if rc:
                        raise RuntimeError(f"pcgrl_rollout rc={rc}")

            # (warm-up past the first episode end: sokoban sizes its solver workspace the first time the solver is seen running)
            run_rollouts(max(1, R // 10, (int(env.cfg.max_iterations) + 1) // GR + 2))
            barrier()
            t1 = time.perf_counter()
            run_rollouts(R)
            barrier()
            el_r, _ = max_over_ranks(time.perf_counter() - t1)
            env.check_errors()
            us = el_r / (R * GR) * 1e6
            rollout = {"value": total_envs * R * GR / el_r, "unit": "env-steps/s", "steps_per_launch": GR, "launches": R,
                       "us_per_step": us, "roofline_frac": ALGO_BYTES[args.workload] * N / (us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                       "form": ("one launch per call" if env._L.pcgrl_rollout_is_one_launch(env._h) == 1 else
                                "issued as step launches by the one call (a 2-D map of more than 16 rows: the one-launch kernel loses to "
                                "stepping there)"),
                       "note": "open-loop action sequences only (actions known in advance); all per-step outputs written; "
                               "measured before the timed region"}
            del obs_r
        return rollout

    def reduce_episodes(after=None, launched=False):
        """the path's only exchange: one pcgrl_reduce_episodes launch (`launched`: it was the last node of the graph just
        replayed); world == 1: the kernel writes its 3 + n_stats doubles straight into pinned host memory (no copy);
        world > 1: one small all-gather over RCCL, then one device -> host copy.  Ends with the device synchronised."""
        if not use_coll:
            rc = 0 if launched else env._L.pcgrl_reduce_episodes(env._h, ep_host.data_ptr(), 1, sptr)
            if rc:
                raise RuntimeError(f"pcgrl_reduce_episodes rc={rc}")
            # (waiting on an event returns ~15 us sooner than the device-wide wait; the synchronise then finds an idle device)
            if after is not None:
                after.record(stream)
            done_ev.record(stream)
            done_ev.synchronize()
            torch.cuda.synchronize(dev)
            return
        # N > 1: ONE collective -- an all-gather of every rank's 3 + n_stats sums (north_star: "a RCCL all-gather over xGMI only for
        # the episodic-return reduction") -- and ONE device -> host copy of the world x (3 + n_stats) doubles; the sum over the
        # ranks, in rank order, is taken on the host.  (Round 4 all-reduced in place and needed one more device copy to keep this
        # rank's own count: every operation behind the K launches is ~8 us of a 170 us region.)
        if not launched:
            env.reduce_episodes(clear=True, out=ep_dev)
        if coll_dev.type == "cpu":  # gloo test hook
            t = ep_dev.cpu()
            parts = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(parts, t)
            ep_all_host.copy_(torch.cat(parts))
            if after is not None:
                after.record(stream)
                torch.cuda.synchronize(dev)
        else:
            dist.all_gather_into_tensor(ep_all_dev, ep_dev)
            if after is not None:
                after.record(stream)
            ep_all_host.copy_(ep_all_dev, non_blocking=True)
            torch.cuda.synchronize(dev)
        allr = ep_all_host.view(world, -1)
        ep_host.copy_(allr.sum(0))
        local_eps[0] = float(allr[rank, 2])

    def measure_closed_loop():
        """Secondary figure: SURVEY 8(d)'s protocol taken literally (profile_env.py:134-139: an action sampled at every step).
        One HIP graph of Gc [pcgrl_sample_actions -> pcgrl_step] pairs -- the sampler is one more kernel per step whose output
        the step launch depends on -- replayed to cover Kc steps; HIP events on the launch stream.  Never `value`."""
        Kc = args.closed_loop_steps if args.closed_loop_steps >= 0 else max(K, 2000)
        if Kc <= 0 or inject is not None or evo or sfg:
            return None
        Gc = min(125, Kc)
        act_buf = torch.empty((N, env.action_entries), dtype=torch.int32, device=dev)
        # (sokoban: how a step is launched while the device solver has recently been seen running -- a workgroup per env plus
        # helper waves, for the next 16 launches -- is a host decision a capture freezes; let it lapse before capturing)
        for _ in range(24):
            env._L.pcgrl_sample_actions(env._h, act_buf.data_ptr(), 1234 + rank, sptr)
            step_raw(act_buf.data_ptr(), sptr)
        torch.cuda.synchronize(dev)
        try:
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream(dev)
            side.wait_stream(stream)
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                    cap = torch.cuda.current_stream(dev).cuda_stream
                    for _ in range(Gc):
                        rc = env._L.pcgrl_sample_actions(env._h, act_buf.data_ptr(), 1234 + rank, cap)
                        rc = rc or step_raw(act_buf.data_ptr(), cap)
                        if rc:
                            raise RuntimeError(f"closed loop (capture) rc={rc}")
            stream.wait_stream(side)
        except Exception as exc:  # noqa: BLE001
            torch.cuda.synchronize(dev)
            return {"error": repr(exc)}
        reps = max(1, Kc // Gc)
        for _ in range(max(1, reps // 10)):
            g.replay()
        barrier()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t1 = time.perf_counter()
        e0.record(stream)
        for _ in range(reps):
            g.replay()
        e1.record(stream)
        barrier()
        el, _ = max_over_ranks(time.perf_counter() - t1)
        env.check_errors()
        us_ev = e0.elapsed_time(e1) / (reps * Gc) * 1e3
        us = el / (reps * Gc) * 1e6
        del g
        return {"value": total_envs * reps * Gc / el, "unit": "env-steps/s", "steps": reps * Gc, "us_per_step": us,
                "us_per_step_hip_events": us_ev, "roofline_frac": ALGO_BYTES[args.workload] * N / (us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                "launch": f"HIP graph of {Gc} [pcgrl_sample_actions -> pcgrl_step] pairs per replay",
                "note": "an action drawn on the device at every step (counter-based generator, draw counter in device memory: fresh "
                        "actions at every replay); two dependent kernels per step; measured after the timed region"}

    def measure_first_replay():
        """Round 4's short-run protocol, kept as a detail: ONE graph of all K steps, uploaded but never launched before the
        clock starts.  Returns ms per step of that first replay (+ the closing synchronise), or None."""
        if not (2 <= K <= 125) or inject is not None or evo or sfg or graph is None or (G == K and not fuse_reduce):
            return None
        try:
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream(dev)
            side.wait_stream(stream)
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                    cap = torch.cuda.current_stream(dev).cuda_stream
                    for k in range(K):
                        if step_raw(base + (k % POOL) * stride, cap):
                            raise RuntimeError("capture")
            stream.wait_stream(side)
            env._L.pcgrl_graph_upload(g.raw_cuda_graph_exec(), stream.cuda_stream)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            g.replay()
            done_ev.record(stream)
            done_ev.synchronize()
            return (time.perf_counter() - t1) / K * 1e3
        except Exception:  # noqa: BLE001
            torch.cuda.synchronize(dev)
            return None

    def measure_fill():
        """What a write-only kernel reaches at this launch size: a device fill of exactly the launch's algorithmic byte
        count (graph of 20 fills, HIP events).  At 13.7 MB (4096 binary envs) a fill ends after ~4.2 us = 0.40 of the
        8 TB/s spec peak -- launch ramp and drain of one short kernel -- and ~0.86 of it from 200 MB up.  Reported next to
        the roofline as context for `frac`; measured before the timed region; never `value`."""
        nbytes = int(ALGO_BYTES[args.workload] * N)
        if rank != 0 or nbytes > (8 << 30):
            return None
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for _ in range(20):
                    buf.fill_(1)
        stream.wait_stream(side)
        reps = max(3, min(50, int(2e-3 / (20 * max(nbytes / 6.5e12, 4e-6)))))
        with torch.cuda.stream(stream):
            for _ in range(3):
                g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                g.replay()
            e1.record(stream)
        torch.cuda.synchronize(dev)
        us = e0.elapsed_time(e1) / (reps * 20) * 1e3
        del g, buf
        return {"bytes": nbytes, "us": us, "GBps": nbytes / us / 1e3, "frac_of_peak": nbytes / us / 1e3 / HBM_PEAK_GBS}

    reduce_episodes()  # warm the reporting path (first collective), clean accumulators
    fill = measure_fill() if not args.dry_run else None
    rollout = measure_rollout()
    run(W)
    reduce_episodes()  # episodes that ended during the warm-up do not count
    if overlap:
        # the warm-up interval's sums of THIS rank: what the side stream gathers while the timed interval steps.  The side
        # stream's first collective (communicator channels, PyTorch's per-stream bookkeeping) happens here, untimed.
        ep_prev_cpu.copy_(ep_all_host.view(world, -1)[rank])
        ep_prev_dev.copy_(ep_prev_cpu)
        torch.cuda.synchronize(dev)
        if coll_dev.type != "cpu":
            with torch.cuda.stream(xstream):
                dist.all_gather_into_tensor(ep_all_dev, ep_prev_dev)
            torch.cuda.synchronize(dev)
    if budget > 0:
        step_raw.rewind()
        status_rows.zero_()
    barrier()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record(stream)
    run(K)
    ev2 = torch.cuda.Event(enable_timing=True)
    exposed_ms = 0.0
    if overlap:
        # N > 1, default.  The region has the N = 1 region's structure -- K step launches, the pcgrl_reduce_episodes launch (the
        # last node of the same graph when the region is one graph), ONE synchronise -- and the only collective of the path, the
        # all-gather of the PREVIOUS interval's sums + its device->host copy, runs on a side stream under the stepping (SURVEY
        # 8 e).  Every reporting interval of a long run looks like this: it reduces its own episodes and ships the previous
        # interval's.  No rank waits for another inside the region; the clock of a rank stops when ITS device is idle, and the
        # figure is the maximum over the ranks.  (The interval's own sums are gathered after the clock, for the report.)
        if not fuse_reduce:
            env.reduce_episodes(clear=True, out=ep_dev)
        ev1.record(stream)
        if coll_dev.type == "cpu":  # gloo test hook: a host-side all-gather while the device steps
            parts = [torch.zeros_like(ep_prev_cpu) for _ in range(world)]
            dist.all_gather(parts, ep_prev_cpu)
            ep_all_host.copy_(torch.cat(parts))
        else:
            with torch.cuda.stream(xstream):
                dist.all_gather_into_tensor(ep_all_dev, ep_prev_dev)
                ep_all_host.copy_(ep_all_dev, non_blocking=True)
                ev_x.record(xstream)
        ev1.synchronize()
        torch.cuda.synchronize(dev)  # (both streams)
        elapsed = time.perf_counter() - t0
        prev_interval = ep_all_host.view(world, -1).sum(0).tolist()  # what the host reads at the end of the region
        if coll_dev.type != "cpu":
            try:  # how long the side stream outlived the stepping stream (0 when it was done first: fully hidden)
                exposed_ms = max(0.0, ev1.elapsed_time(ev_x))
            except Exception:  # noqa: BLE001
                exposed_ms = 0.0
        ev2 = None
        reduce_episodes(None, launched=True)  # untimed: this interval's own sums, for `episodes`
    else:
        ev1.record(stream)
        prev_interval = None
        # serial form (--exchange serial; also N = 1 without a process group, where there is nothing to gather): the closing
        # barrier of the timed region IS the path's exchange -- with N > 1 ranks the all-gather of the episode sums cannot
        # complete on any rank before every rank has contributed, i.e. finished its K launches.
        if fuse_reduce and not use_coll:
            # the whole region was that one graph (K launches + the reduction, which wrote pinned host memory): ev1 is its end.
            # (Every further event record is a marker packet the command processor works through one after the other: three of
            # them behind a 170 us region cost ~5 % of it.)
            ev1.synchronize()
            torch.cuda.synchronize(dev)
            ev2 = None
        else:
            reduce_episodes(ev2, launched=fuse_reduce)
        elapsed = time.perf_counter() - t0
    kernel_ms = ev0.elapsed_time(ev1) / K  # average launch-to-launch time on the launch stream (HIP events)
    # the exchange on this rank's stepping stream: serial form = reduction launch + all-gather (which also waits for the slowest
    # rank); overlapped form = what of the side stream's work was still running when the stepping stream had finished
    exchange_ms = exposed_ms if overlap else (0.0 if ev2 is None else (ev1.elapsed_time(ev2) if ev2.query() else float("nan")))
    env.check_errors()
    emitted_total = None
    if budget > 0:  # asynchronous stepping: the env-steps of the region are the transitions its launches emitted
        st_k = status_rows[:K]
        mine = float((st_k & 1).sum().item())
        _, per_rank_emitted = max_over_ranks(mine)
        emitted_total = sum(per_rank_emitted)
        busy_share = float(((st_k & 2) != 0).float().mean().item())
    elapsed, per_rank_elapsed = max_over_ranks(elapsed)
    _, per_rank_eps = max_over_ranks(float(local_eps[0]))
    _, per_rank_kernel_ms = max_over_ranks(kernel_ms)
    _, per_rank_exchange_ms = max_over_ranks(exchange_ms)
    dumped = None
    if args.dump_outputs:  # before anything else steps this env (the first-replay and closed-loop figures below do)
        f32, f64 = np.float32, np.float64
        if sfg:
            per_env = {"stats": (sfg_out, f64)}
        elif evo:
            per_env = {"obs": (env._obs, f32)}
            if K >= EVO_K:  # (the timed steps restart at update 0: a refresh ran in them only if there were EVO_K of them)
                per_env["stats"] = (env._stats, f64)
        else:
            per_env = {"obs": (env._obs, f32), "reward": (env._reward, f32), "done": (env._done, f32), "stats": (env._stats, f64)}
            if budget > 0:
                per_env["status"] = (status_rows[K - 1], f32)
        dumped = dump_outputs(args.dump_outputs, per_env, {"episode_sums": ep_host.tolist()}, rank, world)
    first_replay_ms = measure_first_replay()
    _, per_rank_first = max_over_ranks(first_replay_ms if first_replay_ms is not None else float("nan"))
    closed = measure_closed_loop()
    h = ep_host.tolist()
    n_ep = max(h[2], 1.0)
    ep = {"episodes": h[2], "mean_return": h[0] / n_ep, "mean_length": h[1] / n_ep,
          "mean_final_stats": [x / n_ep for x in h[3:]]}

    if rank == 0:
        value = total_envs * K / elapsed if emitted_total is None else emitted_total / elapsed
        bytes_per_launch = int(ALGO_BYTES[args.workload] * N) if emitted_total is None else int(ALGO_BYTES[args.workload] * emitted_total / world / K)
        achieved = bytes_per_launch / (elapsed / K) / 1e9          # same clock as `value`
        achieved_ev = bytes_per_launch / (kernel_ms * 1e-3) / 1e9  # HIP events around the K launches
        traffic, traffic_src, profiled_head = profiled_traffic(args.workload, N)
        k_mean_us = profiled_kernel_mean_us(args.workload, N)
        if solver_active and budget == 0:  # (the profiled entry of this workload is the ASYNCHRONOUS kernel: nothing to echo here)
            traffic, traffic_src, profiled_head, k_mean_us = None, "only the asynchronous step kernel of this workload was profiled (--solver-budget 16)", None, None
        out = {
            "metric": "env-steps/sec at N envs/GPU (binary 16x16), 1/2/4/8 MI355X",
            "value": value, "unit": "maps/s" if sfg else "env-steps/s", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": elapsed / K * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u8", "data": "synthetic",
            "config": {"workload": f"{args.workload} {'x'.join(map(str, shape))}, {N} envs/GPU, "
                                   + ("playable levels (one player, 1-3 crates / targets, one room) re-injected every 8 steps, floor / "
                                      "wall edits in and around the room, no auto-reset, "
                                      + (f"ASYNCHRONOUS stepping (pcgrl_step_ready, solver budget {budget} per env and launch: a 'step' of "
                                         "--steps is one launch, value counts emitted transitions), " if budget > 0 else "") if solver_active else
                                      "injected maps with one player / key / door, random moves and empty / solid / enemy "
                                      "placements, no auto-reset, " if bfs_active else
                                      f"evolution-driver pattern (evo/evolve.py:1083-1120): one pcgrl_update launch (rep.update + observation) per "
                                      f"step, one pcgrl_refresh_stats (get_stats) every {EVO_K} steps, uniform random actions, " if evo else
                                      f"Problem.get_stats on {N} caller maps resident in HBM per launch (pcgrl_stats_for_grids_h, evo/evolve.py:1106-1115), "
                                      "maps drawn with a tile distribution of their own each; a 'step' is one launch, value = maps/s, " if sfg else
                                      "uniform random actions, auto-reset, ")
                                   + "uint8 one-hot obs (channel-last)",
                       "envs_per_gpu": N, "global_envs": total_envs, "episode_len": int(env.cfg.max_iterations) + 1,
                       # (SURVEY 8(d) says torch.randint per step; the action source is not the hot path, so the rows are drawn
                       # once, on the device, before the timed region, and step k reads row k mod POOL)
                       "actions": f"pool of {POOL} pre-drawn rows of uniform random actions resident in HBM, row k mod {POOL} at step k",
                       "parallelism": f"env-sharded x{world} (no data-path collective; episodic-return all-gather)",
                       "launch": f"HIP graph of {G} steps per replay" if graph is not None else "eager, one launch per step (issued by pcgrl_step_seq)" if inject is None else "eager, one launch per step",
                       "seed_ranges": [[0x5EED + lo, 0x5EED + hi - 1] for lo, hi in
                                       (shard_env_range(total_envs, r, world) for r in range(world))]},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                         # `traffic` and `kernel_mean_us` are echoes of committed profile files, never measurements of this run:
                         # the commit they were profiled at and the identity of the kernels running now
                         "profiled_at_head": profiled_head, "kernel_sources_sha16": kernel_sources_sha16(_family(args.workload)),
                         "kernel": "pcgrl::m3_kernel" if problem == "minecraft_3D_maze" else "pcgrl::step_kernel (update_only)" if evo
                         else "pcgrl::stats_for_grids_kernel" if sfg else "pcgrl::step_kernel",
                         "algorithmic_bytes_per_launch": bytes_per_launch,
                         "clock": "wall clock of the timed region / steps (the clock of `value`)",
                         "achieved_hip_events": achieved_ev, "frac_hip_events": achieved_ev / HBM_PEAK_GBS,
                         # from the COMMITTED rocprofv3 --kernel-trace mean of the dominant kernel (profiles/r*_summary.json),
                         # begin-to-end of the kernel alone: the figure a reader can recompute from profiles/
                         "kernel_mean_us": k_mean_us,
                         "kernel_frac": (bytes_per_launch / (k_mean_us * 1e-6) / 1e9 / HBM_PEAK_GBS) if k_mean_us else None,
                         "avg_launch_us": kernel_ms * 1e3,
                         # context, not a peak: a device fill of the same byte count on the same GPU in the same run
                         "fill_same_bytes": (dict(fill, step_over_fill=(elapsed / K * 1e6) / fill["us"]) if fill else None)},
            "episodes": ep,
        }
        # per rank: its own clock of the timed region, the HIP-event time of its K launches alone, and the exchange: weak-scaling
        # efficiency can be read off this one line as  min(launch_ms_per_step at N = 1) / max(launch_ms_per_step)
        how = ("" if not use_coll else
               " of the previous interval's sums on a side stream, under the stepping" if overlap else " behind the K launches (closing barrier)")
        out["per_rank"] = {"env_steps_per_s": [N * K / t for t in per_rank_elapsed], "ms_per_step": [t / K * 1e3 for t in per_rank_elapsed],
                           "launch_ms_per_step": per_rank_kernel_ms, "exchange_ms": per_rank_exchange_ms,
                           "episodes": per_rank_eps,
                           "collective": "none" if not use_coll else f"{backend} all-gather of {3 + env.n_stats} doubles per rank" + how
                                         + (" (world size 1: --force-collective)" if world == 1 else ""),
                           "cores": "all" if pinned is None else f"{len(pinned)} per rank (sched_setaffinity by LOCAL_RANK)"}
        if first_replay_ms is not None:  # round 4's protocol for short runs, for comparison (never `value`)
            out["per_rank"]["first_replay_of_one_graph_ms_per_step"] = per_rank_first
        # what the timed region consists of on the slowest rank
        region = (f"ONE replay of a HIP graph of {K} step launches + the pcgrl_reduce_episodes launch "
                  "(uploaded with hipGraphUpload, never launched before; the W warm-up steps are eager launches); `launches_ms` "
                  "includes that reduction launch"
                  if fuse_reduce else
                  f"{W // G} untimed + {K // G} timed replays of one HIP graph of {G} steps" if graph is not None and K < 250 and G and G < K and W % G == 0 and K % G == 0
                  else f"replays of a HIP graph of {G} steps (+ {K % G} eager launches)" if graph is not None
                  else "eager launches")
        out["timed_region"] = {"wall_ms": elapsed * 1e3, "launches_ms": max(per_rank_kernel_ms) * K,
                               "exchange_ms": max(per_rank_exchange_ms), "exchange_share_of_wall": max(per_rank_exchange_ms) / (elapsed * 1e3),
                               "protocol": region}
        if use_coll:
            tr = out["timed_region"]
            tr["exchange"] = args.exchange
            if overlap:
                # Structure check for whoever computes value(N) / (N x value(1)): the share of this region that the N = 1 region
                # (K launches + reduction launch + one synchronise, no process group) has as well.  `exchange_ms` is what of the
                # side stream's all-gather + copy was still running when the stepping stream had finished (0: fully hidden).
                tr["protocol_efficiency_bound"] = max(0.0, 1.0 - tr["exchange_ms"] / tr["wall_ms"])
                tr["structure"] = ("the N = 1 region's: K step launches + the reduction launch + ONE synchronise per rank, maximum over the ranks; "
                                   "the all-gather + device->host copy of the previous interval's sums run on a side stream meanwhile and the "
                                   "host reads them at the end of the region (`previous_interval_sums`); no rank waits for another inside the region")
                tr["previous_interval_sums"] = prev_interval
            else:
                tr["protocol_efficiency_bound"] = max(0.0, 1.0 - tr["exchange_ms"] / tr["wall_ms"])
                tr["structure"] = ("round 5's: reduction -> all-gather -> device->host copy BEHIND the K launches; the N = 1 line's region holds "
                                   "no collective and no copy, so value(N) / (N x value(1)) charges the exchange itself before any loss from adding ranks")
        if closed is not None:
            out["closed_loop_device_actions"] = closed
        if solver_active and budget > 0:
            out["asynchronous_stepping"] = {
                "solver_budget": budget, "launches": K, "emitted_transitions": emitted_total,
                "emitted_share_of_env_launches": emitted_total / (total_envs * K), "busy_share_of_env_launches": busy_share,
                "us_per_launch": elapsed / K * 1e6,
                "note": "pcgrl_step_ready: every launch gives every env's search `solver_budget` iteration units (BFS 1, A* 2), parks "
                        "what is unfinished and reports the env busy; `value` = emitted transitions / s (a busy env does not step); "
                        "per-env trajectories equal the synchronous ones (tests/test_gpu_round6.py)"}
        if solver_active:
            st = env.get_state().stats
            out["solver_active"] = {"reinject_every": REINJECT, "solver_power": int(env.cfg.solver_power),
                                    "envs_with_solver_result_at_end": (st[:, 4] != 8192).float().mean().item(),
                                    "envs_solved_at_end": (st[:, 5] > 0).float().mean().item()}
        elif bfs_active:
            st = env.get_state().stats
            both = ((st[:, 0] == 1) & (st[:, 1] == 1) & (st[:, 2] == 1)).float().mean().item()
            out["bfs_active"] = {"reinject_every": REINJECT, "envs_with_both_searches_at_end": both,
                                 "envs_with_one_player_at_end": (st[:, 0] == 1).float().mean().item()}
        if solver_active and args.solver_forms > 0:
            try:
                out["solver_active_forms"] = solver_forms(problem, rep, shape, N, dev, inject, actions, args.solver_forms, REINJECT)
            except Exception as exc:  # noqa: BLE001
                out["solver_active_forms"] = {"error": repr(exc)}
        if rollout is not None:
            out["open_loop_rollout"] = rollout
        if dumped is not None:
            out["dump_outputs"] = dumped
    if use_coll:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # The CPU baseline runs on rank 0 AFTER the process group is gone: the other ranks have left (none of them sits in a
        # barrier, spinning, while the OpenMP threads are timed) and rank 0 may use every host core again.
        # (secondary figures and the CPU baseline belong to the N = 1 line: "on rank 0 at N = 1 only")
        if world == 1 and (args.rllib_adapter > 0 or (args.rllib_adapter < 0 and args.workload == "binary-narrow" and args.envs == 0)):
            try:  # (a secondary figure must never cost the run its line)
                out["rllib_adapter"] = rllib_adapter_bench(problem, rep, shape, dev)
            except Exception as exc:  # noqa: BLE001
                out["rllib_adapter"] = {"error": repr(exc)}
        if world == 1 and args.sub_batches and inject is None and not evo and not sfg and not wkw:
            try:
                out["async_sub_batches"] = sub_batch_bench(args.workload, problem, rep, shape, N, dev,
                                                           [int(x) for x in args.sub_batches.split(",") if int(x) > 1 and N % int(x) == 0],
                                                           one_batch_us=(out["roofline"]["avg_launch_us"] if K >= 250 else None))
            except Exception as exc:  # noqa: BLE001
                out["async_sub_batches"] = {"error": repr(exc)}
        if not args.no_cpu_baseline and world == 1:
            if pinned is not None:
                try:
                    os.sched_setaffinity(0, all_cores)
                except OSError:
                    pass
            if world > 1:
                time.sleep(1.0)  # (the other ranks tear down their runtimes)
            out["cpu_baseline"] = cpu_baseline(problem, rep, shape, N, args.cpu_seconds, wkw, bfs_active, solver_active, REINJECT,
                                               mode="evo" if evo else "sfg" if sfg else "step", maps=sfg_host if sfg else None)
        try:  # RCCL prints its version banner through C stdio; whatever sits in that buffer goes out BEFORE the line
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:  # noqa: BLE001
            pass
        sys.stderr.flush()
        print(json.dumps(out), flush=True)
    watchdog.cancel()


def gpus_without_runtime():
    """GPUs this process may use, counted from /sys/class/kfd (a node with simd_count > 0 is a GPU) and the *_VISIBLE_DEVICES
    lists -- no HIP / HSA call, so the launcher stays a process that has never opened the GPU.  None = cannot tell."""
    import glob
    n = 0
    files = glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")
    if not files:
        return None
    for f in files:
        try:
            props = dict(line.split()[:2] for line in open(f) if len(line.split()) >= 2)
            n += 1 if int(props.get("simd_count", "0")) > 0 else 0
        except Exception:
            return None
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None and v.strip() != "":
            n = min(n, len([x for x in v.split(",") if x.strip() != ""]))
    return n


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks as child processes (this process never touches
    the GPU), relay rank 0's JSON line, return the worst exit code."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    # rank 0's output is read on a thread so that this loop can watch every rank: one that dies before the rendezvous
    # would otherwise leave the others (and this launcher) waiting for it for ever
    import threading
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    deadline = time.time() + float(os.environ.get("PCGRL_BENCH_TIMEOUT", "3600"))
    failed = None
    while any(p.poll() is None for p in procs):
        bad = [r for r, p in enumerate(procs) if p.poll() not in (None, 0)]
        if bad or time.time() > deadline:
            failed = f"rank {bad[0]} exited with code {procs[bad[0]].returncode}" if bad else "timeout"
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(0.2)
    rcs = [p.wait() for p in procs]
    reader.join(timeout=5)
    sys.stdout.write(b"".join(chunks).decode())
    sys.stdout.flush()
    if failed:
        sys.stderr.write(f"bench.py launcher: {failed}; the remaining ranks were stopped\n")
        return 1
    return max(abs(rc) for rc in rcs)


def solver_forms(problem, rep, shape, n_envs, dev, inject, actions, steps, reinject):
    """The solver-active workload through the two forms that shrink a launch's synchronisation domain WITHOUT a ready mask
    (VERDICT r5 Weak 2): pcgrl_rollout (`reinject` steps per launch between re-injections: waves advance independently, a launch
    waits for the slowest env's SUM over the steps) and sub_batches = 4 (a launch waits for the slowest env of N / 4).
    Synchronous solver, same maps and action rows as the timed region.  Secondary figures, never `value`."""
    import numpy as np
    import torch
    from control_pcgrl_amd import SubBatchedVecEnv, VecPcgrlEnv
    out = {"steps": steps, "reinject_every": reinject, "unit": "env-steps/s"}
    rounds = max(1, steps // reinject)
    stream = torch.cuda.current_stream(dev).cuda_stream
    env = VecPcgrlEnv(problem, rep, shape, n_envs, device=dev, seeds=0x5EED + np.arange(n_envs), auto_reset=False)
    rew = torch.empty((reinject, n_envs), dtype=torch.float32, device=dev)
    done = torch.empty((reinject, n_envs), dtype=torch.uint8, device=dev)
    stats = torch.empty((reinject, n_envs, env.n_stats), dtype=torch.int32, device=dev)
    obs = torch.empty((reinject, n_envs) + env.obs_shape, dtype=torch.uint8, device=dev)

    def rollout_rounds(n, first=0):
        for r in range(first, first + n):
            env._L.pcgrl_reset(env._h, None, inject.data_ptr(), None, stream)
            rc = env._L.pcgrl_rollout(env._h, actions[(r * reinject) % (actions.shape[0] - reinject):].data_ptr(), reinject, 0,
                                      obs.data_ptr(), 0, rew.data_ptr(), done.data_ptr(), stats.data_ptr(), stream)
            if rc:
                raise RuntimeError(f"pcgrl_rollout rc={rc}")
    rollout_rounds(2)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    rollout_rounds(rounds, 2)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    env.check_errors()
    env.close()
    out["pcgrl_rollout"] = {"value": n_envs * rounds * reinject / dt, "us_per_step": dt / (rounds * reinject) * 1e6,
                            "steps_per_launch": reinject}
    sb = SubBatchedVecEnv(problem, rep, shape, n_envs, 4, device=dev, seeds=0x5EED + np.arange(n_envs), auto_reset=False)

    def sb_steps(n, first=0):
        for k in range(first, first + n):
            if k % reinject == 0:
                sb.reset(init_grids=inject)
            sb.step(actions[k % actions.shape[0]])
    sb_steps(2 * reinject)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    sb_steps(rounds * reinject, 2 * reinject)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    sb.check_errors()
    sb.close()
    out["sub_batches_4"] = {"value": n_envs * rounds * reinject / dt, "us_per_step": dt / (rounds * reinject) * 1e6}
    return out


def sub_batch_bench(workload, problem, rep, shape, n_envs, dev, ks, graph_steps=50, replays=20, one_batch_us=None):
    """`async_sub_batches`: a step launch waits for its slowest env; k independent sub-batch chains (k engines, k streams, one
    HIP graph with k parallel branches: control_pcgrl_amd.SubBatchedVecEnv) shrink that synchronisation domain.  Same envs
    (seeds), same action source as the timed region; us per step of the WHOLE batch by HIP events.  Never `value`."""
    import numpy as np
    import torch
    from control_pcgrl_amd import SubBatchedVecEnv, VecPcgrlEnv
    rows = []
    main_s = torch.cuda.current_stream(dev)
    for k in [1] + list(ks):
        if k == 1:
            env = VecPcgrlEnv(problem, rep, shape, n_envs, device=dev, seeds=0x5EED + np.arange(n_envs), auto_reset=True)
        else:
            env = SubBatchedVecEnv(problem, rep, shape, n_envs, k, device=dev, seeds=0x5EED + np.arange(n_envs), auto_reset=True)
        env.reset()
        g = torch.Generator(device=dev).manual_seed(1234)
        acts = torch.randint(0, env.num_actions, (64, n_envs), generator=g, device=dev, dtype=torch.int32)
        for t in range(3):
            env.step(acts[t])
        torch.cuda.synchronize(dev)
        gr = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(dev)
        side.wait_stream(main_s)
        with torch.cuda.stream(side):
            with torch.cuda.graph(gr, stream=side, capture_error_mode="thread_local"):
                if k == 1:
                    for t in range(graph_steps):
                        env.step(acts[t % 64])
                else:  # the chains are independent over the whole graph: sub-batch i's launch t + 1 only follows ITS launch t
                    n = n_envs // k
                    for t in range(graph_steps):
                        for i in range(k):
                            env.step_async(i, acts[t % 64, i * n:(i + 1) * n])
                    env.wait()
        main_s.wait_stream(side)
        for _ in range(4):
            gr.replay()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(main_s)
        for _ in range(replays):
            gr.replay()
        e1.record(main_s)
        torch.cuda.synchronize(dev)
        env.check_errors()
        us = e0.elapsed_time(e1) * 1e3 / (replays * graph_steps)
        rows.append({"sub_batches": k, "us_per_step_of_whole_batch": us, "env_steps_per_s": n_envs / (us * 1e-6),
                     "roofline_frac": ALGO_BYTES[workload] * n_envs / (us * 1e-6) / 1e9 / HBM_PEAK_GBS})
        del gr
        env.close()
    base = rows[0]["us_per_step_of_whole_batch"]
    for r in rows:
        r["speedup_vs_one_batch_same_protocol"] = base / r["us_per_step_of_whole_batch"]
    return {"unit": "env-steps/s", "rows": rows, "graph_steps": graph_steps, "replays": replays,
            "note": "k engines of N / k envs on k streams (SubBatchedVecEnv.step_async): sub-batch i's launch t + 1 only follows ITS launch "
                    "t, so a launch waits for the slowest env of N / k instead of N and the chains overlap on the device; one HIP graph "
                    "with k parallel branches; the first steps of an episode (3-D mazes: slower than the episode average behind `value`)"}


def rllib_adapter_bench(problem, rep, shape, dev, sizes=(20, 2000, 4096), seconds=0.7):
    """The RLlib-shaped boundary (control_pcgrl_amd/rllib_env.py, the reference's fleet is 12 workers x 20 envs:
    rl/utils.py:396-415): env-steps/s of vector_step + the reset_at calls RLlib makes for finished envs, host arrays out,
    random actions from host memory.  Secondary figure, never `value`."""
    import numpy as np
    from control_pcgrl_amd.rllib_env import PcgrlVectorEnv
    cfg = {"task": {"problem": problem, "map_shape": list(shape), "obs_window": None, "weights": None}, "representation": rep}
    rows = []
    for n in sizes:
        for name, direct in (("float32", None), ("uint8", False), ("uint8", True)):
            venv = PcgrlVectorEnv(cfg, num_envs=n, device=dev, seeds=1000 + np.arange(n), obs_dtype=np.dtype(name),
                                  direct_host_outputs=direct)
            venv.vector_reset()
            rng = np.random.default_rng(5)
            acts = [rng.integers(0, venv.vec.num_actions, size=n) for _ in range(16)]

            def loop(limit):
                t0 = time.perf_counter()
                k = resets = 0
                while time.perf_counter() - t0 < limit:
                    obs, rew, done, trunc, infos = venv.vector_step(acts[k % 16])
                    k += 1
                    if any(done):
                        for i in np.nonzero(done)[0]:
                            venv.reset_at(int(i))
                            resets += 1
                return k, resets, time.perf_counter() - t0

            loop(0.15)
            k, resets, dt = loop(seconds)
            rows.append({"envs": n, "obs_dtype": name, "env_steps_per_s": n * k / dt, "host_us_per_vector_step": dt / k * 1e6,
                         "calls": k, "reset_at_calls": resets, "kernel_writes_host_memory": bool(venv._direct),
                         "d2h_bytes_per_call": 0 if venv._direct else int(venv._total), "pinned_blocks": len(venv._free) + 1,
                         "obs_bytes_handed_out_per_call": int(n * np.prod(venv.observation_space.shape) * np.dtype(name).itemsize)})
            venv.close()
    return {"unit": "env-steps/s", "what": "PcgrlVectorEnv.vector_step(actions) -> (obs list, rewards, dones, truncateds, infos) + reset_at for "
            "finished envs; one pcgrl_step launch and one device->host copy per call (or none: kernel_writes_host_memory); the arrays "
            "of a call are never rewritten (a pinned block of their own, recycled when they are garbage)", "rows": rows}


def kernel_sources_sha16(family=None):
    """identity of the kernels a measurement belongs to: sha256 over the sources they are built from (kernel headers, the
    per-problem translation units, the C ABI header with the config struct; not the host side, pcgrl_engine.hip).  family "2d":
    the 2-D problems' kernels (without the 3-D translation unit and header); "3d": everything (the 3-D kernels include the 2-D
    header); None: {"2d": ..., "3d": ...}"""
    import glob
    import hashlib
    if family is None:
        return {"2d": kernel_sources_sha16("2d"), "3d": kernel_sources_sha16("3d")}
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(ROOT, "control_pcgrl_amd", "csrc", "*.h")) + glob.glob(os.path.join(ROOT, "control_pcgrl_amd", "csrc", "*.hip"))
                   + [os.path.join(ROOT, "include", "pcgrl_amd.h")])
    for f in files:
        if family == "2d" and os.path.basename(f) in ("pcgrl_kernels3d.h", "pcgrl_k_3d.hip"):
            continue
        if os.path.basename(f) == "pcgrl_engine.hip":  # (host side: argument checks, allocation, launches -- not the profiled kernels)
            continue
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def _family(workload):
    return "3d" if "3D" in workload else "2d"


def _profile_summaries(workload):
    """committed rocprofv3 summaries, oldest first, each with whether it was taken on THESE kernels (of the workload's family)"""
    import glob
    fam = _family(workload)
    cur = kernel_sources_sha16(fam)
    out = []
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_summary.json"))):
        try:
            s = json.load(open(f))
        except Exception:
            continue
        h = s.get("kernel_sources_sha16")
        out.append((f, s, isinstance(h, dict) and h.get(fam) == cur))
    return out, cur


def profiled_traffic(workload, n_envs):
    """HBM bytes per launch of the step kernel from the committed rocprofv3 --pmc passes of this same command
    (profiles/r*_summary.json: WRITE_SIZE + 2 x FETCH_SIZE), where the number comes from and the
    commit it was profiled at.  Counters cannot be collected inside a timing run, so this is an ECHO of a committed file -- and
    only of one taken on the kernels that are running: a summary whose `kernel_sources_sha16` differs from the sources of this
    checkout is refused (None, with the reason)."""
    sums, cur = _profile_summaries(workload)
    best, stale = (None, None, None), None
    for f, s, same in sums:
        rec = s.get("hbm_traffic_per_launch_by_workload", {}).get(f"{workload}@{n_envs}")
        if rec is None:
            continue
        rel = os.path.relpath(f, ROOT)
        if same:
            best = (rec["traffic_bytes"], rel + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes)", s.get("profiled_at_head"))
        else:
            stale = rel
    if best[0] is None and stale is not None:
        return None, f"{stale} was taken on other kernels (kernel_sources_sha16 != {cur}): not echoed", None
    return best


def profiled_kernel_mean_us(workload, n_envs):
    """mean begin-to-end duration of the dominant kernel in the committed rocprofv3 kernel trace of this workload at its
    default batch, taken on the kernels of this checkout (see profiled_traffic), or None"""
    best = None
    if n_envs != WORKLOADS[workload][3]:
        return None
    for f, s, same in _profile_summaries(workload)[0]:
        if not same:
            continue
        try:
            d = s["workloads"].get(workload, {}).get("dominant_kernel_launch")
            if d:
                best = d["duration_ns"]["mean"] / 1e3
        except Exception:
            pass
    return best


def cpu_baseline(problem, rep, shape, n_envs, target_s, wkw=None, bfs_active=False, solver_active=False, reinject=128,
                 mode="step", maps=None):
    """The oracle (a C port of the reference's algorithm, OpenMP over envs) on the host cores of this box:
    same workload, bounded sample."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pcgrl_oracle as po
    avail = os.cpu_count() or 1
    try:
        avail = len(os.sched_getaffinity(0))
    except Exception:
        pass
    try:  # honour a cgroup CPU quota (containers often expose more cores than they may use)
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            avail = max(1, min(avail, int(int(quota) / int(period))))
    except Exception:
        pass
    os.environ.setdefault("OMP_WAIT_POLICY", "passive")

    def rate_sfg(threads, seconds):  # Problem.get_stats over the same maps, OpenMP over maps
        t0 = time.perf_counter()
        steps = 0
        sub = maps[:max(2048, min(len(maps), 4096 * threads))]
        while True:
            po.stats_for_grids(problem, sub.reshape((len(sub),) + tuple(shape)), threads=threads)
            steps += 1
            if time.perf_counter() - t0 > seconds:
                break
        dt = time.perf_counter() - t0
        return len(sub) * steps / dt, steps, dt

    def rate_evo(threads, seconds):  # n_cells x rep.update (+ observation), then one get_stats, OpenMP over envs
        orc = po.OracleVecEnv(problem, rep, shape, n_envs, seeds=0x5EED + np.arange(n_envs), threads=threads)
        orc.reset()
        period = int(np.prod(shape))
        t0 = time.perf_counter()
        steps = 0
        while True:
            orc.update(acts[steps % 64])
            steps += 1
            if steps % period == 0:
                orc.refresh_stats()
            if steps >= 5 and time.perf_counter() - t0 > seconds:
                break
        dt = time.perf_counter() - t0
        return n_envs * steps / dt, steps, dt

    def rate(threads, seconds):
        if mode == "sfg":
            return rate_sfg(threads, seconds)
        if mode == "evo":
            return rate_evo(threads, seconds)
        orc = po.OracleVecEnv(problem, rep, shape, n_envs, seeds=0x5EED + np.arange(n_envs), threads=threads,
                              **(wkw or {}))
        maps = sa_maps if solver_active else (bfs_active_maps(n_envs, 77) if bfs_active else None)
        if maps is not None:
            orc.reset(init_grids=maps)
        else:
            orc.reset()
        for k in range(2):
            orc.step(acts[k], auto_reset=not bfs_active)
        t0 = time.perf_counter()
        steps = 0
        while True:
            if maps is not None and steps % reinject == 0:
                orc.reset(init_grids=maps)
            orc.step(acts[steps % 64], auto_reset=not bfs_active)
            steps += 1
            if steps >= 5 and time.perf_counter() - t0 > seconds:
                break
        dt = time.perf_counter() - t0
        return n_envs * steps / dt, steps, dt

    rng = np.random.default_rng(1234)
    n_act = {"narrow": po.N_TILES[problem], "turtle": po.N_TILES[problem] + 4,
             "wide": int(np.prod(shape)) * po.N_TILES[problem]}[rep]
    entries = int(np.prod(wkw["act_window"])) if wkw and wkw.get("act_window") else 1
    acts = rng.integers(0, n_act, size=(64, n_envs * entries), dtype=np.int32)
    sa_maps = None
    if solver_active:
        sa_maps, sa_cells = solver_active_maps(n_envs, 77)
        acts = solver_active_actions(sa_cells, 64, 1234)
    elif bfs_active:
        acts = np.array(BFS_ACTIONS, np.int32)[rng.integers(0, len(BFS_ACTIONS), size=(64, n_envs))]
    # pick the thread count that this box actually rewards (short calibration), then time the sample
    # (>= 2 s per candidate: shorter calibrations picked 8 threads for one workload where every other picked 16)
    cands = sorted({avail, max(1, avail // 2), min(avail, 32)})
    best_threads, best_rate = 1, 0.0
    for th in cands:
        r, _, _ = rate(th, 2.0)
        if r > best_rate:
            best_threads, best_rate = th, r
    value, steps, dt = rate(best_threads, target_s)
    one_core, _, _ = rate(1, 1.5)
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except Exception:
        pass
    return {"value": value, "unit": "maps/s" if mode == "sfg" else "env-steps/s", "cores": best_threads, "cpu_model": model,
            "usable_cores": avail, "kind": "port", "one_core": one_core,
            "sample": (f"{steps} passes of Problem.get_stats over a {min(len(maps), 4096 * best_threads)}-map slice of the same maps "
                       f"({dt:.1f} s, OpenMP over maps with {best_threads} threads of {avail} usable cores)" if mode == "sfg" else
                       f"{steps} steps x {n_envs} envs of the same workload ({dt:.1f} s, OpenMP over envs with "
                       f"{best_threads} threads of {avail} usable cores, obs encoded as uint8)")}


if __name__ == "__main__":
    main()
