"""MiniDungeon levels on the device: the eleven statistics of MDungeonProblem.get_stats (probs/mdungeon/mdungeon_prob.py:151-171)
-- six counts and scans of the map and, for a level with one player, one exit and one region, the four-stage play-through of
probs/mdungeon/mdungeon/engine.py (A* at balance 1, 0.5 and 0, then BFS) -- for a batch of maps in one launch, the returned
node's move list, the reward and the episode end of the problem, and the level measures, the pairwise Hamming diversity and the
behaviour vector the reference's quality-diversity loop places a level by (include/pcgrl_amd_mdungeon.h,
csrc/mdungeon/pcgrl_mdungeon.h).

This module evaluates and measures maps; stepping MiniDungeon environments is not built (the reference cannot construct the
problem, so no episode could be recorded to pin one against).  It is not part of the 2-D engine, so PROBLEMS / problem_spec /
build_config / make_vec_env do not know "mdungeon".  file:line references are relative to the reference's control_pcgrl/envs/
directory.
"""
import ctypes as C
import math

import torch

from . import _lib
from .ddave import _range_reward
from .measures import MeasuresMixin
from .problems import ProblemSpec

MDUNGEON_TILES = ["empty", "solid", "player", "exit", "potion", "treasure", "goblin", "ogre"]  # mdungeon_prob.py:50-51
MDUNGEON_STAT_KEYS = ["player", "exit", "potions", "treasures", "enemies", "regions", "col-potions", "col-treasures",
                      "col-enemies", "dist-win", "sol-length"]  # get_stats' dict order, mdungeon_prob.py:153-165
MDUNGEON_MOVES = ((-1, 0), (1, 0), (0, -1), (0, 1))  # engine.py:3 directions as (x, y): left, right, up, down
# get_reward's order of summation (mdungeon_prob.py:197-205); col-potions and col-treasures have no term
MDUNGEON_REWARD_ORDER = ("player", "exit", "enemies", "treasures", "potions", "regions", "col-enemies", "dist-win",
                         "sol-length")
MDUNGEON_WEIGHTS = {"player": 3, "exit": 3, "potions": 1, "treasures": 1, "enemies": 2, "regions": 5, "col-enemies": 2,
                    "dist-win": 0.1, "sol-length": 1}  # mdungeon_prob.py:32-42
MDUNGEON_PLAY_KEYS = ("status", "iterations-1", "iterations-2", "iterations-3", "iterations-4", "x", "y", "health",
                      "col_potions", "col_treasures", "col_enemies", "depth")
MDUNGEON_MEASURE_NAMES = ("emptiness", "entropy", "symmetry", "symmetry-horizontal", "symmetry-vertical", "co-occurance")
# what behaviour() takes: get_bc (evo/evolve.py:606-635) looks in the statistics first, then among the measures of the map
MDUNGEON_BC_NAMES = tuple(MDUNGEON_STAT_KEYS) + MDUNGEON_MEASURE_NAMES + ("NONE",)
MAX_H, MAX_W, MAX_SOLVER_POWER, MAX_ITEMS = 16, 32, 16000, 64


def mdungeon_spec(map_shape=(11, 7)) -> ProblemSpec:
    """The problem's tables.  MDungeonProblem has no static targets and no conditional bounds of its own (it predates the
    control wrapper): the reward's ranges live in get_reward (mdungeon_prob.py:185-195) and MDungeonEvaluator.reward."""
    return ProblemSpec("mdungeon", list(MDUNGEON_TILES), list(MDUNGEON_STAT_KEYS), {}, {}, dict(MDUNGEON_WEIGHTS),
                       dict(MDUNGEON_WEIGHTS))


def mdungeon_config(map_shape=(11, 7), solver_power=5000, weights=None, max_enemies=6, max_potions=2, max_treasures=3,
                    target_col_enemies=0.5, target_solution=20) -> "_lib.PcgrlMdungeonConfig":
    """The C config of include/pcgrl_amd_mdungeon.h; `weights` replaces entries of the stock table as adjust_param's
    `rewards` does (mdungeon_prob.py:81-85)."""
    w = dict(MDUNGEON_WEIGHTS)
    unknown = set(weights or {}) - set(w)
    if unknown:
        raise ValueError(f"unknown mdungeon statistics in weights: {sorted(unknown)}")
    w.update(weights or {})
    cfg = _lib.PcgrlMdungeonConfig()
    cfg.h, cfg.w, cfg.solver_power = int(map_shape[0]), int(map_shape[1]), int(solver_power)
    cfg.max_enemies, cfg.max_potions, cfg.max_treasures = int(max_enemies), int(max_potions), int(max_treasures)
    cfg.target_solution, cfg.target_col_enemies = int(target_solution), float(target_col_enemies)
    for i, k in enumerate(MDUNGEON_REWARD_ORDER):
        cfg.weight[i] = float(w[k])
    return cfg


class MDungeonEvaluator(MeasuresMixin):
    """Evaluates batches of MiniDungeon maps (1..16 rows x 1..32 columns) on one device.  Owns the search workspace: per level
    20 * (4 * solver_power + 1) bytes of nodes and open list and 12 bytes for each of the C >= 2 * solver_power slots of the
    visited set -- 596 640 bytes at the stock power of 5 000 (C = 16 384), 2.4 GB for max_levels = 4 096.
    Batches above max_levels run as successive launches on the current stream.  No host sync and no CPU fallback."""

    def __init__(self, map_shape=(11, 7), device="cuda:0", solver_power=5000, weights=None, max_enemies=6, max_potions=2,
                 max_treasures=3, target_col_enemies=0.5, target_solution=20, max_levels=4096):
        self._L = _lib.lib()
        map_shape = tuple(int(s) for s in map_shape)
        if len(map_shape) != 2:
            raise ValueError(f"mdungeon maps are 2-D, got shape {map_shape}")
        if int(max_levels) < 1:
            raise ValueError("max_levels must be at least 1")
        self.map_shape = map_shape
        self.spec = mdungeon_spec(map_shape)
        self.solver_power = int(solver_power)
        self.max_levels = int(max_levels)
        self.max_enemies, self.max_potions, self.max_treasures = int(max_enemies), int(max_potions), int(max_treasures)
        self.target_col_enemies, self.target_solution = float(target_col_enemies), int(target_solution)
        self._cfg = mdungeon_config(map_shape, solver_power, weights, max_enemies, max_potions, max_treasures,
                                    target_col_enemies, target_solution)
        self.weights = {k: self._cfg.weight[i] for i, k in enumerate(MDUNGEON_REWARD_ORDER)}
        nbytes = self._L.pcgrl_mdungeon_workspace_bytes(self.max_levels, map_shape[0], map_shape[1], self.solver_power)
        if nbytes < 0:
            raise NotImplementedError(f"mdungeon: map_shape {map_shape} / solver_power {solver_power} outside 1..{MAX_H} x "
                                      f"1..{MAX_W} and 1..{MAX_SOLVER_POWER}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("MDungeonEvaluator needs a cuda device: there is no CPU fallback")
        self._workspace = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)
        self._workspace_bytes = nbytes
        self._error = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _grids_arg(self, grids):
        if self._workspace is None:
            raise RuntimeError("MDungeonEvaluator is closed")
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
        tensors: stats int32 [n][11] (MDUNGEON_STAT_KEYS order), play int32 [n][12] (MDUNGEON_PLAY_KEYS: status -1 not
        searched, 0 no stage won, 1..4 the stage that won, 5 more than 64 items; the four stages' iterations; the returned
        node's x, y, health, col_potions, col_treasures, col_enemies and depth), length int32 [n] (the returned node's number
        of moves, whatever move_cap cuts), won bool [n], error int32 [n], and with move_cap > 0: moves int8 [n][move_cap]
        (indices into MDUNGEON_MOVES, -1 past the end)."""
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
                _lib.check(self._L.pcgrl_mdungeon_evaluate(
                    C.byref(self._cfg), m, g[lo:].data_ptr(), self._workspace.data_ptr(), self._workspace_bytes, move_cap,
                    ptr("stats", lo), ptr("moves", lo), ptr("length", lo), ptr("play", lo), err[lo:].data_ptr(), stream),
                    "pcgrl_mdungeon_evaluate")
        self._error |= err.max()
        out["error"] = err
        status = out["play"][:, 0]
        out["won"] = (status >= 1) & (status <= 4)
        return out

    def _stats_arg(self, stats):
        s = torch.as_tensor(stats, device=self.device)
        if s.dim() == 1:
            s = s.unsqueeze(0)
        if s.dim() != 2 or s.shape[1] != len(MDUNGEON_STAT_KEYS):
            raise ValueError(f"stats must have shape [n, {len(MDUNGEON_STAT_KEYS)}], got {list(s.shape)}")
        return s

    def reward(self, new_stats, old_stats):
        """MDungeonProblem.get_reward (mdungeon_prob.py:183-205) of n pairs of statistics ([n, 11], evaluate()'s stats):
        float64 [n], equal to the reference's value bit for bit -- get_range_reward per statistic with the reference's bounds
        (+-inf among them), each term one multiplication by its weight, added in the reference's order.  torch expressions on
        the current stream (a multiplication and an addition are two kernels: nothing is fused); no host sync."""
        new, old = self._stats_arg(new_stats).to(torch.float64), self._stats_arg(old_stats).to(torch.float64)
        if new.shape != old.shape:
            raise ValueError("new_stats and old_stats must have the same shape")
        inf = math.inf
        bounds = {"player": (1, 1), "exit": (1, 1), "potions": (-inf, self.max_potions), "treasures": (-inf, self.max_treasures),
                  "enemies": (1, self.max_enemies), "regions": (1, 1), "col-enemies": (inf, inf), "dist-win": (-inf, -inf),
                  "sol-length": (inf, inf)}
        total = None
        for k in MDUNGEON_REWARD_ORDER:
            j = MDUNGEON_STAT_KEYS.index(k)
            term = _range_reward(new[:, j], old[:, j], *bounds[k]) * self.weights[k]
            total = term if total is None else total + term
        return total

    def episode_over(self, stats):
        """MDungeonProblem.get_episode_over (mdungeon_prob.py:218-221): bool [n]; the share of enemies met is a float64
        division, as the reference's"""
        s = self._stats_arg(stats)
        enemies = s[:, 4]
        share = s[:, 8].to(torch.float64) / torch.clamp(enemies, min=1).to(torch.float64)
        return (s[:, 10] >= self.target_solution) & (enemies > 0) & (share > self.target_col_enemies)

    def check_errors(self):
        """Raises if a launch of evaluate() since the last check read a tile id above 7 (it was taken as solid).  Synchronises.
        measures() / diversity() mask ids to 3 bits and set no error."""
        bits = int(self._error.item())
        self._error.zero_()
        if bits & 1:
            raise ValueError("mdungeon: a tile id above 7 was seen on the device (read as solid)")

    def _meas_dims(self):
        return self.map_shape[0] * self.map_shape[1], len(MDUNGEON_TILES)

    def measures(self, grids, entropy=True):
        """The behaviour characteristics of the maps that the reference computes from the integer map (evo/evolve.py:606-635
        get_bc -> :423-592), as LodeRunnerEvaluator.measures returns them with T = 8: counts int32 [n, 8], match int32 [n, 3]
        (horizontal, vertical, wrapped co-occurance matches), forms float64 [n, 12], tile_fractions float64 [n, 8] and bc, a
        dict under get_bc's names -> float64 [n] (also .entropy, .emptiness).  The divisors are the map's own H * W.  grids:
        uint8 [n][H][W] at any alignment, n >= 0; ids are masked to 3 bits and set no error.  One launch on the current stream,
        no host sync."""
        g = self._grids_arg(grids)
        H, W, n = *self.map_shape, g.shape[0]
        return self._measures_result(self._L.pcgrl_mdungeon_measures_for_grids, (H, W, n, g.data_ptr()), n, entropy)

    def diversity(self, grids, group=None, pairwise=False):
        """Pairwise Hamming distances (cells whose tiles differ) among the maps in consecutive groups of `group` maps (None: one
        group of all), as LodeRunnerEvaluator.diversity returns them: hamming_sum int64 [G], scores float64 [G, 2], nearest /
        nearest_idx int32 [n] (the lowest index on ties), div_score and diversity_bonus float64 [G], pairwise int32 [G, K, K]
        or None.  Three launches on the current stream, no host sync."""
        g = self._grids_arg(grids)
        H, W, n = *self.map_shape, g.shape[0]
        return self._diversity_result(self._L.pcgrl_mdungeon_diversity_for_grids, (H, W, n, g.data_ptr()), n, group, pairwise,
                                      self._L.pcgrl_mdungeon_diversity_scratch_bytes(H, W, n))

    def behaviour(self, grids, names):
        """The behaviour vector of each map: float64 [n, len(names)], column j the reference's get_bc(names[j], ...)
        (evo/evolve.py:606-635).  A name among MDUNGEON_STAT_KEYS is that column of evaluate()'s stats (get_bc looks there
        first); a name of MDUNGEON_MEASURE_NAMES is the measure of that name; "NONE" is 0.  evaluate(move_cap=0) runs only if a
        statistic is named, the measures launch only if a measure is named, and the entropy is computed only if named.  No host
        sync."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [k for k in names if k not in MDUNGEON_BC_NAMES]
        if unknown:
            raise ValueError(f"unknown behaviour characteristics {unknown}: the known names are {list(MDUNGEON_BC_NAMES)}")
        g = self._grids_arg(grids)
        stats = self.evaluate(g, move_cap=0)["stats"] if any(k in MDUNGEON_STAT_KEYS for k in names) else None
        meas = self.measures(g, entropy="entropy" in names).bc if any(k in MDUNGEON_MEASURE_NAMES for k in names) else None
        out = torch.zeros((g.shape[0], len(names)), dtype=torch.float64, device=self.device)
        for j, k in enumerate(names):
            if k in MDUNGEON_STAT_KEYS:
                out[:, j] = stats[:, MDUNGEON_STAT_KEYS.index(k)]
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
