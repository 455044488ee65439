"""Dangerous Dave levels on the device: the eleven statistics of DDaveProblem.get_stats (probs/ddave/ddave_prob.py:149-169) --
seven counts and scans of the map and, for a level with one player, one exit, one key and one region, the four-stage
play-through of probs/ddave/ddave/engine.py (A* at balance 1, 0.5 and 0, then BFS) -- for a batch of maps in one launch, the
returned node's action list, the reward and the episode end of the problem, and the level measures, the pairwise Hamming
diversity and the behaviour vector the reference's quality-diversity loop places a level by (include/pcgrl_amd_ddave.h,
csrc/ddave/pcgrl_ddave.h).

This module evaluates and measures maps; stepping Dangerous Dave environments is not built (the reference cannot construct the
problem, so no episode could be recorded to pin one against).  It is not part of the 2-D engine, so PROBLEMS / problem_spec /
build_config / make_vec_env do not know "ddave".  file:line references are relative to the reference's control_pcgrl/envs/
directory.
"""
import ctypes as C
import math

import torch

from . import _lib
from .measures import MeasuresMixin
from .problems import ProblemSpec

DDAVE_TILES = ["empty", "solid", "player", "exit", "diamond", "key", "spike"]  # ddave_prob.py:53-54
DDAVE_STAT_KEYS = ["player", "dist-floor", "exit", "diamonds", "key", "spikes", "regions", "num-jumps", "col-diamonds",
                   "dist-win", "sol-length"]  # get_stats' dict order, ddave_prob.py:151-163
DDAVE_MOVES = ((0, 0), (-1, 0), (1, 0), (0, -1))  # engine.py:3 directions as (x, y): stay, left, right, jump
# get_reward's order of summation (ddave_prob.py:196-205); col-diamonds has no term
DDAVE_REWARD_ORDER = ("player", "dist-floor", "exit", "spikes", "diamonds", "key", "regions", "num-jumps", "dist-win",
                      "sol-length")
DDAVE_WEIGHTS = {"player": 3, "dist-floor": 2, "exit": 3, "diamonds": 1, "key": 3, "spikes": 1, "regions": 5, "num-jumps": 3,
                 "dist-win": 0.1, "sol-length": 1}  # ddave_prob.py:31-42
DDAVE_PLAY_KEYS = ("status", "iterations-1", "iterations-2", "iterations-3", "iterations-4", "x", "y", "airTime", "health",
                   "col_key", "diamonds", "depth")
DDAVE_MEASURE_NAMES = ("emptiness", "entropy", "symmetry", "symmetry-horizontal", "symmetry-vertical", "co-occurance")
# what behaviour() takes: get_bc (evo/evolve.py:606-635) looks in the statistics first, then among the measures of the map
DDAVE_BC_NAMES = tuple(DDAVE_STAT_KEYS) + DDAVE_MEASURE_NAMES + ("NONE",)
MAX_H, MAX_W, MAX_SOLVER_POWER, MAX_DIAMONDS = 16, 32, 16000, 64


def ddave_spec(map_shape=(7, 11)) -> ProblemSpec:
    """The problem's tables.  DDaveProblem has no static targets and no conditional bounds of its own (it predates the
    control wrapper): the reward's ranges live in get_reward (ddave_prob.py:184-193) and DDaveEvaluator.reward."""
    return ProblemSpec("ddave", list(DDAVE_TILES), list(DDAVE_STAT_KEYS), {}, {}, dict(DDAVE_WEIGHTS), dict(DDAVE_WEIGHTS))


def ddave_config(map_shape=(7, 11), solver_power=5000, weights=None, max_diamonds=3, min_spikes=10, target_jumps=2,
                 target_solution=20) -> "_lib.PcgrlDdaveConfig":
    """The C config of include/pcgrl_amd_ddave.h; `weights` replaces entries of the stock table as adjust_param's `rewards`
    does (ddave_prob.py:83-87)."""
    w = dict(DDAVE_WEIGHTS)
    unknown = set(weights or {}) - set(w)
    if unknown:
        raise ValueError(f"unknown ddave statistics in weights: {sorted(unknown)}")
    w.update(weights or {})
    cfg = _lib.PcgrlDdaveConfig()
    cfg.h, cfg.w, cfg.solver_power = int(map_shape[0]), int(map_shape[1]), int(solver_power)
    cfg.max_diamonds, cfg.min_spikes = int(max_diamonds), int(min_spikes)
    cfg.target_jumps, cfg.target_solution = int(target_jumps), int(target_solution)
    for i, k in enumerate(DDAVE_REWARD_ORDER):
        cfg.weight[i] = float(w[k])
    return cfg


def _range_reward(new, old, low, high):
    """get_range_reward (helper.py:550-560) on float64 tensors of integer values; low and high are Python numbers, infinite
    ones included.  With an infinite bound some branches cannot be taken and the rest collapse: what is left is written out, so
    no inf - inf is ever formed."""
    inf = math.inf
    if low == inf or high == -inf:  # nothing is in range: with both bounds +inf the `<= high` branch, with -inf the `>= low`
        return new - old if low == inf else old - new
    if low == -inf and high == inf:
        return torch.zeros_like(new)
    if low == -inf:  # `>= low` holds always; in range both maxima are `high`
        return torch.clamp(old, min=high) - torch.clamp(new, min=high)
    if high == inf:
        return torch.clamp(new, max=low) - torch.clamp(old, max=low)
    zero = torch.zeros_like(new)
    both_in = (new >= low) & (new <= high) & (old >= low) & (old <= high)
    r = torch.where(new > high, high - new + old - low, high - old + new - low)  # the two crossings
    r = torch.where((old >= low) & (new >= low), torch.clamp(old, min=high) - torch.clamp(new, min=high), r)
    r = torch.where((old <= high) & (new <= high), torch.clamp(new, max=low) - torch.clamp(old, max=low), r)
    return torch.where(both_in, zero, r)


class DDaveEvaluator(MeasuresMixin):
    """Evaluates batches of Dangerous Dave maps (1..16 rows x 1..32 columns) on one device.  Owns the search workspace: per
    level 20 * (4 * solver_power + 1) bytes of nodes and open list and 12 bytes for each of the C >= 2 * solver_power slots of
    the visited set -- 596 640 bytes at the stock power of 5 000 (C = 16 384), 2.4 GB for max_levels = 4 096.
    Batches above max_levels run as successive launches on the current stream.  No host sync and no CPU fallback."""

    def __init__(self, map_shape=(7, 11), device="cuda:0", solver_power=5000, weights=None, max_diamonds=3, min_spikes=10,
                 target_jumps=2, target_solution=20, max_levels=4096):
        self._L = _lib.lib()
        map_shape = tuple(int(s) for s in map_shape)
        if len(map_shape) != 2:
            raise ValueError(f"ddave maps are 2-D, got shape {map_shape}")
        if int(max_levels) < 1:
            raise ValueError("max_levels must be at least 1")
        self.map_shape = map_shape
        self.spec = ddave_spec(map_shape)
        self.solver_power = int(solver_power)
        self.max_levels = int(max_levels)
        self.max_diamonds, self.min_spikes = int(max_diamonds), int(min_spikes)
        self.target_jumps, self.target_solution = int(target_jumps), int(target_solution)
        self._cfg = ddave_config(map_shape, solver_power, weights, max_diamonds, min_spikes, target_jumps, target_solution)
        self.weights = {k: self._cfg.weight[i] for i, k in enumerate(DDAVE_REWARD_ORDER)}
        nbytes = self._L.pcgrl_ddave_workspace_bytes(self.max_levels, map_shape[0], map_shape[1], self.solver_power)
        if nbytes < 0:
            raise NotImplementedError(f"ddave: map_shape {map_shape} / solver_power {solver_power} outside 1..{MAX_H} x "
                                      f"1..{MAX_W} and 1..{MAX_SOLVER_POWER}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("DDaveEvaluator needs a cuda device: there is no CPU fallback")
        self._workspace = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)
        self._workspace_bytes = nbytes
        self._error = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _grids_arg(self, grids):
        if self._workspace is None:
            raise RuntimeError("DDaveEvaluator is closed")
        g = torch.as_tensor(grids, device=self.device)
        if g.dtype != torch.uint8:
            g = g.to(torch.uint8)
        if g.dim() == 2:
            g = g.unsqueeze(0)
        if g.dim() != 3 or tuple(g.shape[1:]) != self.map_shape:
            raise ValueError(f"grids must have shape [n]{list(self.map_shape)}, got {list(g.shape)}")
        return g.contiguous()

    def evaluate(self, grids, move_cap=0):
        """grids: uint8 [n][H][W] (a device tensor at any alignment, or anything torch.as_tensor takes).  Returns device
        tensors: stats int32 [n][11] (DDAVE_STAT_KEYS order), play int32 [n][12] (DDAVE_PLAY_KEYS: status -1 not searched, 0 no
        stage won, 1..4 the stage that won, 5 more than 64 diamonds; the four stages' iterations; the returned node's x, y,
        airTime, health, col_key; the diamonds in the level; the returned node's depth), length int32 [n] (the returned node's
        number of actions, whatever move_cap cuts), won bool [n], error int32 [n], and with move_cap > 0: moves int8
        [n][move_cap] (indices into DDAVE_MOVES, -1 past the end)."""
        g = self._grids_arg(grids)
        n = g.shape[0]
        if n < 1:
            raise ValueError("no levels to evaluate")
        move_cap = int(move_cap)
        if move_cap < 0:
            raise ValueError("move_cap must not be negative")
        dev = self.device
        out = {"stats": torch.empty((n, 11), dtype=torch.int32, device=dev),
               "play": torch.empty((n, 12), dtype=torch.int32, device=dev),
               "length": torch.empty(n, dtype=torch.int32, device=dev)}
        if move_cap > 0:
            out["moves"] = torch.empty((n, move_cap), dtype=torch.int8, device=dev)
        err = torch.empty(n, dtype=torch.int32, device=dev)

        def ptr(name, lo):
            return out[name][lo:].data_ptr() if name in out else None

        with torch.cuda.device(dev):
            stream = self._stream()
            for lo in range(0, n, self.max_levels):
                m = min(self.max_levels, n - lo)
                _lib.check(self._L.pcgrl_ddave_evaluate(
                    C.byref(self._cfg), m, g[lo:].data_ptr(), self._workspace.data_ptr(), self._workspace_bytes, move_cap,
                    ptr("stats", lo), ptr("moves", lo), ptr("length", lo), ptr("play", lo), err[lo:].data_ptr(), stream),
                    "pcgrl_ddave_evaluate")
        self._error |= err.max()
        out["error"] = err
        status = out["play"][:, 0]
        out["won"] = (status >= 1) & (status <= 4)
        return out

    def _stats_arg(self, stats):
        s = torch.as_tensor(stats, device=self.device)
        if s.dim() == 1:
            s = s.unsqueeze(0)
        if s.dim() != 2 or s.shape[1] != len(DDAVE_STAT_KEYS):
            raise ValueError(f"stats must have shape [n, {len(DDAVE_STAT_KEYS)}], got {list(s.shape)}")
        return s

    def reward(self, new_stats, old_stats):
        """DDaveProblem.get_reward (ddave_prob.py:181-205) of n pairs of statistics ([n, 11], evaluate()'s stats): float64
        [n], equal to the reference's value bit for bit -- get_range_reward per statistic with the reference's bounds
        (+-inf among them), each term one multiplication by its weight, added in the reference's order.  torch expressions on
        the current stream (a multiplication and an addition are two kernels: nothing is fused); no host sync."""
        new, old = self._stats_arg(new_stats).to(torch.float64), self._stats_arg(old_stats).to(torch.float64)
        if new.shape != old.shape:
            raise ValueError("new_stats and old_stats must have the same shape")
        inf = math.inf
        bounds = {"player": (1, 1), "exit": (1, 1), "diamonds": (-inf, self.max_diamonds), "dist-floor": (0, 0), "key": (1, 1),
                  "spikes": (self.min_spikes, inf), "regions": (1, 1), "num-jumps": (inf, inf), "dist-win": (-inf, -inf),
                  "sol-length": (inf, inf)}
        total = None
        for k in DDAVE_REWARD_ORDER:
            j = DDAVE_STAT_KEYS.index(k)
            term = _range_reward(new[:, j], old[:, j], *bounds[k]) * self.weights[k]
            total = term if total is None else total + term
        return total

    def episode_over(self, stats):
        """DDaveProblem.get_episode_over (ddave_prob.py:218-220): bool [n]"""
        s = self._stats_arg(stats)
        return (s[:, 10] >= self.target_solution) & (s[:, 7] > self.target_jumps)

    def check_errors(self):
        """Raises if a launch of evaluate() since the last check read a tile id above 6 (it was taken as solid).  Synchronises.
        measures() / diversity() mask ids to 3 bits and set no error."""
        bits = int(self._error.item())
        self._error.zero_()
        if bits & 1:
            raise ValueError("ddave: a tile id above 6 was seen on the device (read as solid)")

    def _meas_dims(self):
        return self.map_shape[0] * self.map_shape[1], len(DDAVE_TILES)

    def measures(self, grids, entropy=True):
        """The behaviour characteristics of the maps that the reference computes from the integer map (evo/evolve.py:606-635
        get_bc -> :423-592), as LodeRunnerEvaluator.measures returns them with T = 7: counts int32 [n, 7], match int32 [n, 3]
        (horizontal, vertical, wrapped co-occurance matches), forms float64 [n, 12], tile_fractions float64 [n, 7] and bc, a
        dict under get_bc's names -> float64 [n] (also .entropy, .emptiness).  The divisors are the map's own H * W.  grids:
        uint8 [n][H][W] at any alignment, n >= 0; ids are masked to 3 bits and set no error.  One launch on the current stream,
        no host sync."""
        g = self._grids_arg(grids)
        H, W, n = *self.map_shape, g.shape[0]
        return self._measures_result(self._L.pcgrl_ddave_measures_for_grids, (H, W, n, g.data_ptr()), n, entropy)

    def diversity(self, grids, group=None, pairwise=False):
        """Pairwise Hamming distances (cells whose tiles differ) among the maps in consecutive groups of `group` maps (None: one
        group of all), as LodeRunnerEvaluator.diversity returns them: hamming_sum int64 [G], scores float64 [G, 2], nearest /
        nearest_idx int32 [n] (the lowest index on ties), div_score and diversity_bonus float64 [G], pairwise int32 [G, K, K]
        or None.  Three launches on the current stream, no host sync."""
        g = self._grids_arg(grids)
        H, W, n = *self.map_shape, g.shape[0]
        return self._diversity_result(self._L.pcgrl_ddave_diversity_for_grids, (H, W, n, g.data_ptr()), n, group, pairwise,
                                      self._L.pcgrl_ddave_diversity_scratch_bytes(H, W, n))

    def behaviour(self, grids, names):
        """The behaviour vector of each map: float64 [n, len(names)], column j the reference's get_bc(names[j], ...)
        (evo/evolve.py:606-635).  A name among DDAVE_STAT_KEYS is that column of evaluate()'s stats (get_bc looks there first);
        a name of DDAVE_MEASURE_NAMES is the measure of that name; "NONE" is 0.  evaluate(move_cap=0) runs only if a statistic
        is named, the measures launch only if a measure is named, and the entropy is computed only if named.  No host sync."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [k for k in names if k not in DDAVE_BC_NAMES]
        if unknown:
            raise ValueError(f"unknown behaviour characteristics {unknown}: the known names are {list(DDAVE_BC_NAMES)}")
        g = self._grids_arg(grids)
        stats = self.evaluate(g, move_cap=0)["stats"] if any(k in DDAVE_STAT_KEYS for k in names) else None
        meas = self.measures(g, entropy="entropy" in names).bc if any(k in DDAVE_MEASURE_NAMES for k in names) else None
        out = torch.zeros((g.shape[0], len(names)), dtype=torch.float64, device=self.device)
        for j, k in enumerate(names):
            if k in DDAVE_STAT_KEYS:
                out[:, j] = stats[:, DDAVE_STAT_KEYS.index(k)]
            elif k != "NONE":
                out[:, j] = meas[k]
        return out

    def close(self):
        self._workspace = None
        self._entropy_tab = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
