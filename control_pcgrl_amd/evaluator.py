"""What the level evaluators share (SmbEvaluator, LodeRunnerEvaluator, MicrostructureEvaluator, the play-through games'
PlaythroughEvaluator and, in part, Mc3dHoleyEvaluator): the constructor checks, the grids argument, the batched launch that
splits a batch at max_levels, the level measures, diversity and behaviour vector over the family's tables, the error word and
close() -- written once over a family's class attributes.  The workspace stays the family's own: the
classes' docstrings say why they differ.  file:line references are relative to the reference's control_pcgrl/ directory."""
import ctypes as C

import torch

from . import _lib
from .measures import MeasuresMixin


class EvaluatorCore:
    """What needs no table of a family, and so serves Mc3dHoleyEvaluator too: the map shape's rank, the device and the error
    word, the grids argument, close() and the context manager.  RANK is the rank of a map.  A constructor checks
    the shape first (_map_shape_arg; `maps` is how the refusal calls the maps), refuses what it can without a device, then _open(device),
    then allocates; its workspace, if it has one, is _workspace."""

    RANK = 2
    _workspace = None

    def _map_shape_arg(self, map_shape, maps):
        self._L = _lib.lib()
        map_shape = tuple(int(s) for s in map_shape)
        if len(map_shape) != self.RANK:
            raise ValueError(f"{maps} are {self.RANK}-D, got shape {map_shape}")
        return map_shape

    def _open(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} needs a cuda device: there is no CPU fallback")
        self._closed = False
        self._error = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _grids_arg(self, grids):
        """uint8 [n] + map_shape on the device, contiguous; one map stands for a batch of one"""
        if self._closed:
            raise RuntimeError(f"{type(self).__name__} is closed")
        g = torch.as_tensor(grids, device=self.device)
        if g.dtype != torch.uint8:
            g = g.to(torch.uint8)
        if g.dim() == self.RANK:
            g = g.unsqueeze(0)
        if g.dim() != self.RANK + 1 or tuple(g.shape[1:]) != self.map_shape:
            raise ValueError(f"grids must have shape [n]{list(self.map_shape)}, got {list(g.shape)}")
        return g.contiguous()

    def _levels_arg(self, grids):
        g = self._grids_arg(grids)
        if g.shape[0] < 1:
            raise ValueError("no levels to evaluate")
        return g

    def close(self):
        self._closed = True
        self._workspace = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class LevelEvaluator(EvaluatorCore, MeasuresMixin):
    """The base of the evaluators of 2-D levels.  A family sets NAME (the C ABI's pcgrl_<NAME>_* calls), TILES,
    STAT_KEYS, MEASURE_NAMES and BC_NAMES (what behaviour() takes), STATS_ONLY (the cap keyword that, at 0, leaves evaluate()
    the statistics alone) and TILE_READ_AS (what a tile id above the last tile is taken as, for check_errors' text).  Its
    constructor calls this one first, builds spec and _cfg, refuses what it can without a device, then _open(device), then
    allocates."""

    NAME = TILES = STAT_KEYS = MEASURE_NAMES = BC_NAMES = STATS_ONLY = TILE_READ_AS = None

    def __init__(self, map_shape, max_levels):
        self.map_shape = self._map_shape_arg(map_shape, f"{self.NAME} maps")
        if int(max_levels) < 1:
            raise ValueError("max_levels must be at least 1")
        self.max_levels = int(max_levels)

    def _call(self, what):
        return getattr(self._L, f"pcgrl_{self.NAME}_{what}")

    def _launch(self, fn, g, head, out, names):
        """fn(_cfg, m, grids, *head, outputs..., error, stream) over the levels of g, max_levels of them a launch, on the
        current stream.  `names`: the outputs in fn's order; one that `out` does not have, or that is empty, goes as NULL.
        ORs the levels' error words into _error and returns them (int32 [n])."""
        n, dev = g.shape[0], self.device
        err = torch.empty(n, dtype=torch.int32, device=dev)
        outs = [out[k] if k in out and out[k].numel() else None for k in names]
        with torch.cuda.device(dev):
            stream = self._stream()
            for lo in range(0, n, self.max_levels):
                m = min(self.max_levels, n - lo)
                ptrs = [None if t is None else t[lo:].data_ptr() for t in outs]
                _lib.check(fn(C.byref(self._cfg), m, g[lo:].data_ptr(), *head, *ptrs, err[lo:].data_ptr(), stream),
                           fn.__name__)
        self._error |= err.max()
        return err

    def check_errors(self):
        """Raises if a launch of evaluate() (or routes()) since the last check read a tile id that is no tile of the family
        (it was taken as TILE_READ_AS).  Synchronises.  measures() / diversity() mask the ids and set no error."""
        bits = int(self._error.item())
        self._error.zero_()
        if bits & 1:
            raise ValueError(f"{self.NAME}: a tile id above {len(self.TILES) - 1} was seen on the device (read as "
                             f"{self.TILE_READ_AS})")

    def _meas_dims(self):
        return self.map_shape[0] * self.map_shape[1], len(self.TILES)

    def measures(self, grids, entropy=True):
        """The behaviour characteristics of the maps that the reference computes from the integer map (evo/evolve.py:606-635
        get_bc -> :423-592), as VecPcgrlEnv.measures returns them with T = len(TILES): counts int32 [n, T], match int32 [n, 3]
        (horizontal, vertical, wrapped co-occurance matches), forms float64 [n, 5 + T], tile_fractions float64 [n, T] and bc,
        a dict under get_bc's names -> float64 [n] (also .entropy, .emptiness).  All but entropy equal the reference bit for
        bit; entropy does on the host whose numpy built the table.  The divisors are the map's own H * W.  grids: uint8
        [n][H][W] at any alignment, n >= 0; ids are masked to the bits of T - 1 and set no error.  One launch on the current
        stream, no host sync."""
        g = self._grids_arg(grids)
        H, W, n = *self.map_shape, g.shape[0]
        return self._measures_result(self._call("measures_for_grids"), (H, W, n, g.data_ptr()), n, entropy)

    def diversity(self, grids, group=None, pairwise=False):
        """Pairwise Hamming distances (cells whose tiles differ) among the maps in consecutive groups of `group` maps (None: one
        group of all), as VecPcgrlEnv.diversity returns them: hamming_sum int64 [G], scores float64 [G, 2], nearest /
        nearest_idx int32 [n] (the lowest index on ties), div_score (rl/evaluate_ctrl.py:42-48) and diversity_bonus
        (evo/evolve.py:1236-1244) float64 [G], pairwise int32 [G, K, K] or None.  Three launches on the current stream, no
        host sync."""
        g = self._grids_arg(grids)
        H, W, n = *self.map_shape, g.shape[0]
        return self._diversity_result(self._call("diversity_for_grids"), (H, W, n, g.data_ptr()), n, group, pairwise,
                                      self._call("diversity_scratch_bytes")(H, W, n))

    def behaviour(self, grids, names):
        """The behaviour vector of each map: float64 [n, len(names)], column j the reference's get_bc(names[j], ...)
        (evo/evolve.py:606-635).  A name among STAT_KEYS is that column of evaluate()'s stats (get_bc looks there first); a
        name of MEASURE_NAMES is the measure of that name; "NONE" is 0.  evaluate(<STATS_ONLY>=0) runs only if a statistic is
        named, the measures launch only if a measure is named, and the entropy is computed only if named.  No host sync."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [k for k in names if k not in self.BC_NAMES]
        if unknown:
            raise ValueError(f"unknown behaviour characteristics {unknown}: the known names are {list(self.BC_NAMES)}")
        g = self._grids_arg(grids)
        stats = self.evaluate(g, **{self.STATS_ONLY: 0})["stats"] if any(k in self.STAT_KEYS for k in names) else None
        meas = self.measures(g, entropy="entropy" in names).bc if any(k in self.MEASURE_NAMES for k in names) else None
        out = torch.zeros((g.shape[0], len(names)), dtype=torch.float64, device=self.device)
        for j, k in enumerate(names):
            if k in self.STAT_KEYS:
                out[:, j] = stats[:, self.STAT_KEYS.index(k)]
            elif k != "NONE":
                out[:, j] = meas[k]
        return out

    def close(self):
        super().close()
        self._entropy_tab = None
