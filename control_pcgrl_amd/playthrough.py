"""What the evaluators of the solver play-through games share (Dangerous Dave, ddave.py; MiniDungeon, mdungeon.py) beyond
what every level evaluator has from evaluator.py's LevelEvaluator: the workspace, the play-through evaluate() and the reward's
summation -- written once over a game's tables (csrc/playthrough/pcgrl_playthrough.h is the device side, DESIGN.md sections
39 and 43).  file:line references are relative to the reference's control_pcgrl/envs/ directory."""
import math

import torch

from .evaluator import LevelEvaluator

MAX_H, MAX_W, MAX_SOLVER_POWER = 16, 32, 16000


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


class PlaythroughEvaluator(LevelEvaluator):
    """The base of DDaveEvaluator and MDungeonEvaluator.  A game sets NAME (the C ABI's pcgrl_<NAME>_* calls), TILES, STAT_KEYS,
    REWARD_ORDER, MEASURE_NAMES and BC_NAMES, and has _bounds() -- the reward's range per statistic -- and episode_over().
    The workspace is allocated once, for max_levels levels.  A tile id that is no tile of the game reads as solid and sets
    the error of evaluate(); measures() / diversity() mask ids to 3 bits."""

    REWARD_ORDER = None
    STATS_ONLY, TILE_READ_AS = "move_cap", "solid"

    def __init__(self, map_shape, device, solver_power, max_levels, spec, cfg):
        """spec and cfg: the game's <name>_spec and <name>_config, the latter closed over the game's parameters"""
        super().__init__(map_shape, max_levels)
        map_shape = self.map_shape
        self.spec = spec(map_shape)
        self.solver_power = int(solver_power)
        self._cfg = cfg(map_shape, solver_power)
        self.weights = {k: self._cfg.weight[i] for i, k in enumerate(self.REWARD_ORDER)}
        nbytes = self._call("workspace_bytes")(self.max_levels, map_shape[0], map_shape[1], self.solver_power)
        if nbytes < 0:
            raise NotImplementedError(f"{self.NAME}: map_shape {map_shape} / solver_power {solver_power} outside 1..{MAX_H} x "
                                      f"1..{MAX_W} and 1..{MAX_SOLVER_POWER}")
        self._open(device)
        self._workspace = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)
        self._workspace_bytes = nbytes

    def evaluate(self, grids, move_cap=0):
        """grids: uint8 [n][H][W] (a device tensor at any alignment, or anything torch.as_tensor takes).  Returns device
        tensors: stats int32 [n][11] (the game's STAT_KEYS order), play int32 [n][12] (the game's play keys, which its class
        describes: status -1 not searched, 0 no stage won, 1..4 the stage that won, 5 more than 64 items; the four stages'
        iterations; the returned node), length int32 [n] (the returned node's number of moves, whatever move_cap cuts), won
        bool [n], error int32 [n], and with move_cap > 0: moves int8 [n][move_cap] (indices into the game's moves, -1 past the
        end)."""
        g = self._levels_arg(grids)
        n, dev = g.shape[0], self.device
        move_cap = int(move_cap)
        if move_cap < 0:
            raise ValueError("move_cap must not be negative")
        out = {"stats": torch.empty((n, 11), dtype=torch.int32, device=dev),
               "play": torch.empty((n, 12), dtype=torch.int32, device=dev),
               "length": torch.empty(n, dtype=torch.int32, device=dev)}
        if move_cap > 0:
            out["moves"] = torch.empty((n, move_cap), dtype=torch.int8, device=dev)
        out["error"] = self._launch(self._call("evaluate"), g, (self._workspace.data_ptr(), self._workspace_bytes, move_cap),
                                    out, ("stats", "moves", "length", "play"))
        status = out["play"][:, 0]
        out["won"] = (status >= 1) & (status <= 4)
        return out

    def _stats_arg(self, stats):
        s = torch.as_tensor(stats, device=self.device)
        if s.dim() == 1:
            s = s.unsqueeze(0)
        if s.dim() != 2 or s.shape[1] != len(self.STAT_KEYS):
            raise ValueError(f"stats must have shape [n, {len(self.STAT_KEYS)}], got {list(s.shape)}")
        return s

    def reward(self, new_stats, old_stats):
        """The problem's get_reward of n pairs of statistics ([n, 11], evaluate()'s stats): float64 [n], equal to the
        reference's value bit for bit -- get_range_reward per statistic with the reference's bounds (+-inf among them; the
        game's _bounds), each term one multiplication by its weight, added in the reference's order (REWARD_ORDER).  torch
        expressions on the current stream (a multiplication and an addition are two kernels: nothing is fused); no host sync."""
        new, old = self._stats_arg(new_stats).to(torch.float64), self._stats_arg(old_stats).to(torch.float64)
        if new.shape != old.shape:
            raise ValueError("new_stats and old_stats must have the same shape")
        bounds = self._bounds()
        total = None
        for k in self.REWARD_ORDER:
            j = self.STAT_KEYS.index(k)
            term = _range_reward(new[:, j], old[:, j], *bounds[k]) * self.weights[k]
            total = term if total is None else total + term
        return total
