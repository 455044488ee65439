"""What the evaluators of the solver play-through games share (Dangerous Dave, ddave.py; MiniDungeon, mdungeon.py): the
workspace and error word, the batched evaluate() call, the reward's summation, and the level measures, diversity and behaviour
vector -- written once over a game's tables (csrc/playthrough/pcgrl_playthrough.h is the device side).
file:line references are relative to the reference's control_pcgrl/envs/ directory."""
import ctypes as C
import math

import torch

from . import _lib
from .measures import MeasuresMixin

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


class PlaythroughEvaluator(MeasuresMixin):
    """The base of DDaveEvaluator and MDungeonEvaluator.  A game sets NAME (the C ABI's pcgrl_<NAME>_* calls), TILES, STAT_KEYS,
    REWARD_ORDER, MEASURE_NAMES and BC_NAMES, and has _bounds() -- the reward's range per statistic -- and episode_over()."""

    NAME = TILES = STAT_KEYS = REWARD_ORDER = MEASURE_NAMES = BC_NAMES = None

    def __init__(self, map_shape, device, solver_power, max_levels, spec, cfg):
        """spec and cfg: the game's <name>_spec and <name>_config, the latter closed over the game's parameters"""
        self._L = _lib.lib()
        map_shape = tuple(int(s) for s in map_shape)
        if len(map_shape) != 2:
            raise ValueError(f"{self.NAME} maps are 2-D, got shape {map_shape}")
        if int(max_levels) < 1:
            raise ValueError("max_levels must be at least 1")
        self.map_shape = map_shape
        self.spec = spec(map_shape)
        self.solver_power = int(solver_power)
        self.max_levels = int(max_levels)
        self._cfg = cfg(map_shape, solver_power)
        self.weights = {k: self._cfg.weight[i] for i, k in enumerate(self.REWARD_ORDER)}
        nbytes = self._call("workspace_bytes")(self.max_levels, map_shape[0], map_shape[1], self.solver_power)
        if nbytes < 0:
            raise NotImplementedError(f"{self.NAME}: map_shape {map_shape} / solver_power {solver_power} outside 1..{MAX_H} x "
                                      f"1..{MAX_W} and 1..{MAX_SOLVER_POWER}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} needs a cuda device: there is no CPU fallback")
        self._workspace = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)
        self._workspace_bytes = nbytes
        self._error = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _call(self, what):
        return getattr(self._L, f"pcgrl_{self.NAME}_{what}")

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _grids_arg(self, grids):
        if self._workspace is None:
            raise RuntimeError(f"{type(self).__name__} is closed")
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
        tensors: stats int32 [n][11] (the game's STAT_KEYS order), play int32 [n][12] (the game's play keys, which its class
        describes: status -1 not searched, 0 no stage won, 1..4 the stage that won, 5 more than 64 items; the four stages'
        iterations; the returned node), length int32 [n] (the returned node's number of moves, whatever move_cap cuts), won
        bool [n], error int32 [n], and with move_cap > 0: moves int8 [n][move_cap] (indices into the game's moves, -1 past the
        end)."""
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

        fn = self._call("evaluate")
        with torch.cuda.device(dev):
            stream = self._stream()
            for lo in range(0, n, self.max_levels):
                m = min(self.max_levels, n - lo)
                _lib.check(fn(C.byref(self._cfg), m, g[lo:].data_ptr(), self._workspace.data_ptr(), self._workspace_bytes,
                              move_cap, ptr("stats", lo), ptr("moves", lo), ptr("length", lo), ptr("play", lo),
                              err[lo:].data_ptr(), stream), f"pcgrl_{self.NAME}_evaluate")
        self._error |= err.max()
        out["error"] = err
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

    def check_errors(self):
        """Raises if a launch of evaluate() since the last check read a tile id that is no tile of the game (it was taken as
        solid).  Synchronises.  measures() / diversity() mask ids to 3 bits and set no error."""
        bits = int(self._error.item())
        self._error.zero_()
        if bits & 1:
            raise ValueError(f"{self.NAME}: a tile id above {len(self.TILES) - 1} was seen on the device (read as solid)")

    def _meas_dims(self):
        return self.map_shape[0] * self.map_shape[1], len(self.TILES)

    def measures(self, grids, entropy=True):
        """The behaviour characteristics of the maps that the reference computes from the integer map (evo/evolve.py:606-635
        get_bc -> :423-592), as LodeRunnerEvaluator.measures returns them with T = len(TILES): counts int32 [n, T], match int32
        [n, 3] (horizontal, vertical, wrapped co-occurance matches), forms float64 [n, 12], tile_fractions float64 [n, T] and
        bc, a dict under get_bc's names -> float64 [n] (also .entropy, .emptiness).  The divisors are the map's own H * W.
        grids: uint8 [n][H][W] at any alignment, n >= 0; ids are masked to 3 bits and set no error.  One launch on the current
        stream, no host sync."""
        g = self._grids_arg(grids)
        H, W, n = *self.map_shape, g.shape[0]
        return self._measures_result(self._call("measures_for_grids"), (H, W, n, g.data_ptr()), n, entropy)

    def diversity(self, grids, group=None, pairwise=False):
        """Pairwise Hamming distances (cells whose tiles differ) among the maps in consecutive groups of `group` maps (None: one
        group of all), as LodeRunnerEvaluator.diversity returns them: hamming_sum int64 [G], scores float64 [G, 2], nearest /
        nearest_idx int32 [n] (the lowest index on ties), div_score and diversity_bonus float64 [G], pairwise int32 [G, K, K]
        or None.  Three launches on the current stream, no host sync."""
        g = self._grids_arg(grids)
        H, W, n = *self.map_shape, g.shape[0]
        return self._diversity_result(self._call("diversity_for_grids"), (H, W, n, g.data_ptr()), n, group, pairwise,
                                      self._call("diversity_scratch_bytes")(H, W, n))

    def behaviour(self, grids, names):
        """The behaviour vector of each map: float64 [n, len(names)], column j the reference's get_bc(names[j], ...)
        (evo/evolve.py:606-635).  A name among STAT_KEYS is that column of evaluate()'s stats (get_bc looks there first); a
        name of MEASURE_NAMES is the measure of that name; "NONE" is 0.  evaluate(move_cap=0) runs only if a statistic is
        named, the measures launch only if a measure is named, and the entropy is computed only if named.  No host sync."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [k for k in names if k not in self.BC_NAMES]
        if unknown:
            raise ValueError(f"unknown behaviour characteristics {unknown}: the known names are {list(self.BC_NAMES)}")
        g = self._grids_arg(grids)
        stats = self.evaluate(g, move_cap=0)["stats"] if any(k in self.STAT_KEYS for k in names) else None
        meas = self.measures(g, entropy="entropy" in names).bc if any(k in self.MEASURE_NAMES for k in names) else None
        out = torch.zeros((g.shape[0], len(names)), dtype=torch.float64, device=self.device)
        for j, k in enumerate(names):
            if k in self.STAT_KEYS:
                out[:, j] = stats[:, self.STAT_KEYS.index(k)]
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
