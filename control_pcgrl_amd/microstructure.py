"""Microstructure levels on the device: the two statistics of MicroStructureProblem.get_stats (`path-length` and `tortuosity`,
helper.py:278-318 calc_tortuosity over the empty cells of a two-phase map), the loss ControlWrapper.get_loss would derive from
them and the per-region record behind both, for a batch of maps in one launch; and the level measures, the pairwise Hamming
diversity and the behaviour vector the reference's quality-diversity loop places a level by (include/pcgrl_amd_microstructure.h,
csrc/microstructure/pcgrl_microstructure.h).

This module evaluates and measures maps; stepping microstructure environments is not built (the reference cannot construct the
problem, so no episode could be recorded to pin one against).  It is not part of the 2-D engine, so PROBLEMS / problem_spec /
build_config / make_vec_env do not know "microstructure".  file:line references are relative to the reference's
control_pcgrl/envs/ directory.
"""
import ctypes as C
import math

import torch

from . import _lib
from .measures import MeasuresMixin
from .problems import ProblemSpec, target_interval

MICROSTRUCTURE_TILES = ["empty", "solid"]  # probs/microstructure/microstructure_prob.py:60-61
MICROSTRUCTURE_STAT_KEYS = ["path-length", "tortuosity"]
MICROSTRUCTURE_MEASURE_NAMES = ("emptiness", "entropy", "symmetry", "symmetry-horizontal", "symmetry-vertical", "co-occurance")
# what behaviour() takes: get_bc (evo/evolve.py:606-635) looks in the statistics first, then among the measures of the map
MICROSTRUCTURE_BC_NAMES = tuple(MICROSTRUCTURE_STAT_KEYS) + MICROSTRUCTURE_MEASURE_NAMES + ("NONE",)
MAX_H, MAX_W = 64, 64


def microstructure_spec(map_shape=(64, 64)) -> ProblemSpec:
    """microstructure_prob.py:17-18 sets _width = _height = 64 BEFORE :32-51 derive the target and the bounds, so those are
    frozen at the stock size whatever the map.  path-length has a bound and no target."""
    fw, fh = 64, 64
    max_path = float(math.ceil(fw / 2) * fh + math.floor(fh / 2))  # 2080.0
    max_tort = max_path / 2  # 1040.0
    weights = {"tortuosity": 1}  # microstructure_prob.py:24-29 _reward_weights
    return ProblemSpec(
        "microstructure", list(MICROSTRUCTURE_TILES), list(MICROSTRUCTURE_STAT_KEYS),
        {"tortuosity": max_tort},
        {"path-length": (0, max_path), "tortuosity": (0, max_tort)},
        dict(weights), dict(weights),
    )


def microstructure_config(map_shape=(64, 64), weights=None) -> "_lib.PcgrlMicrostructureConfig":
    """The C config of include/pcgrl_amd_microstructure.h: the frozen target as a zero-loss interval, and the weights.  A
    statistic without a target (path-length) adds nothing to the loss whatever its weight."""
    spec = microstructure_spec(map_shape)
    weights = dict(spec.default_weights) if weights is None else dict(weights)
    unknown = set(weights) - set(spec.stat_keys)
    if unknown:
        raise ValueError(f"unknown microstructure statistics in weights: {sorted(unknown)}")
    cfg = _lib.PcgrlMicrostructureConfig()
    cfg.h, cfg.w = int(map_shape[0]), int(map_shape[1])
    for i, k in enumerate(spec.stat_keys):
        cfg.weight[i] = float(weights.get(k, 0.0))
        if k in spec.static_trgs:
            cfg.has_trg[i] = 1
            cfg.trg_lo[i], cfg.trg_hi[i] = target_interval(spec.static_trgs[k])
    return cfg


class MicrostructureEvaluator(MeasuresMixin):
    """Evaluates batches of microstructure maps (1..64 rows x 1..64 columns) on one device.  The kernel needs no workspace;
    batches above max_levels run as successive launches on the current stream.  No host sync and no CPU fallback."""

    def __init__(self, map_shape=(64, 64), device="cuda:0", weights=None, max_levels=4096):
        self._L = _lib.lib()
        map_shape = tuple(int(s) for s in map_shape)
        if len(map_shape) != 2:
            raise ValueError(f"microstructure maps are 2-D, got shape {map_shape}")
        if int(max_levels) < 1:
            raise ValueError("max_levels must be at least 1")
        self.map_shape = map_shape
        self.spec = microstructure_spec(map_shape)
        self.max_levels = int(max_levels)
        self._cfg = microstructure_config(map_shape, weights)
        if not (1 <= map_shape[0] <= MAX_H and 1 <= map_shape[1] <= MAX_W):
            raise NotImplementedError(f"microstructure: map_shape {map_shape} outside 1..{MAX_H} x 1..{MAX_W}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("MicrostructureEvaluator needs a cuda device: there is no CPU fallback")
        self._closed = False
        self._error = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _grids_arg(self, grids):
        if self._closed:
            raise RuntimeError("MicrostructureEvaluator is closed")
        g = torch.as_tensor(grids, device=self.device)
        if g.dtype != torch.uint8:
            g = g.to(torch.uint8)
        if g.dim() == 2:
            g = g.unsqueeze(0)
        if g.dim() != 3 or tuple(g.shape[1:]) != self.map_shape:
            raise ValueError(f"grids must have shape [n]{list(self.map_shape)}, got {list(g.shape)}")
        return g.contiguous()

    def evaluate(self, grids, region_cap=0):
        """grids: uint8 [n][H][W] (a device tensor at any alignment, or anything torch.as_tensor takes).  Returns device
        tensors: stats float64 [n][2] (spec.stat_keys order; path_length and tortuosity are views of its columns), loss float64
        [n], regions int32 [n] (the number of regions, the mean's divisor), error int32 [n], and with region_cap > 0:
        region_rec int16 [n][region_cap][5] (per region in visit order start row, start column, far row, far column, d; -1
        past the last region) and region_tort float64 [n][region_cap] (0 past it).  The totals stay complete when region_cap
        is smaller than the number of regions."""
        g = self._grids_arg(grids)
        n = g.shape[0]
        if n < 1:
            raise ValueError("no levels to evaluate")
        region_cap = int(region_cap)
        if region_cap < 0:
            raise ValueError("region_cap must not be negative")
        dev = self.device
        out = {"stats": torch.empty((n, 2), dtype=torch.float64, device=dev),
               "loss": torch.empty(n, dtype=torch.float64, device=dev),
               "regions": torch.empty(n, dtype=torch.int32, device=dev)}
        if region_cap > 0:
            out["region_rec"] = torch.empty((n, region_cap, 5), dtype=torch.int16, device=dev)
            out["region_tort"] = torch.empty((n, region_cap), dtype=torch.float64, device=dev)
        err = torch.empty(n, dtype=torch.int32, device=dev)

        def ptr(name, lo):
            return out[name][lo:].data_ptr() if name in out else None

        with torch.cuda.device(dev):
            stream = self._stream()
            for lo in range(0, n, self.max_levels):
                m = min(self.max_levels, n - lo)
                _lib.check(self._L.pcgrl_microstructure_evaluate(
                    C.byref(self._cfg), m, g[lo:].data_ptr(), region_cap, ptr("stats", lo), ptr("loss", lo), ptr("regions", lo),
                    ptr("region_rec", lo), ptr("region_tort", lo), err[lo:].data_ptr(), stream), "pcgrl_microstructure_evaluate")
        self._error |= err.max()
        out["error"] = err
        out["path_length"] = out["stats"][:, 0]
        out["tortuosity"] = out["stats"][:, 1]
        return out

    def check_errors(self):
        """Raises if a launch of evaluate() since the last check read a tile id above 1 (it was taken as solid).  Synchronises.
        measures() / diversity() mask ids to 1 bit and set no error."""
        bits = int(self._error.item())
        self._error.zero_()
        if bits & 1:
            raise ValueError("microstructure: a tile id above 1 was seen on the device (read as solid)")

    def _meas_dims(self):
        return self.map_shape[0] * self.map_shape[1], len(MICROSTRUCTURE_TILES)

    def measures(self, grids, entropy=True):
        """The behaviour characteristics of the maps that the reference computes from the integer map (evo/evolve.py:606-635
        get_bc -> :423-592), as LodeRunnerEvaluator.measures returns them with T = 2: counts int32 [n, 2], match int32 [n, 3]
        (horizontal, vertical, wrapped co-occurance matches), forms float64 [n, 7], tile_fractions float64 [n, 2] and bc, a
        dict under get_bc's names -> float64 [n] (also .entropy, .emptiness).  The divisors are the map's own H * W.  grids:
        uint8 [n][H][W] at any alignment, n >= 0; ids are masked to 1 bit and set no error.  One launch on the current stream,
        no host sync."""
        g = self._grids_arg(grids)
        H, W, n = *self.map_shape, g.shape[0]
        return self._measures_result(self._L.pcgrl_microstructure_measures_for_grids, (H, W, n, g.data_ptr()), n, entropy)

    def diversity(self, grids, group=None, pairwise=False):
        """Pairwise Hamming distances (cells whose tiles differ) among the maps in consecutive groups of `group` maps (None: one
        group of all), as LodeRunnerEvaluator.diversity returns them: hamming_sum int64 [G], scores float64 [G, 2], nearest /
        nearest_idx int32 [n] (the lowest index on ties), div_score and diversity_bonus float64 [G], pairwise int32 [G, K, K]
        or None.  Three launches on the current stream, no host sync."""
        g = self._grids_arg(grids)
        H, W, n = *self.map_shape, g.shape[0]
        return self._diversity_result(self._L.pcgrl_microstructure_diversity_for_grids, (H, W, n, g.data_ptr()), n, group,
                                      pairwise, self._L.pcgrl_microstructure_diversity_scratch_bytes(H, W, n))

    def behaviour(self, grids, names):
        """The behaviour vector of each map: float64 [n, len(names)], column j the reference's get_bc(names[j], ...)
        (evo/evolve.py:606-635).  A name among spec.stat_keys is that column of evaluate()'s stats (get_bc looks there first); a
        name of MICROSTRUCTURE_MEASURE_NAMES is the measure of that name; "NONE" is 0.  evaluate(region_cap=0) runs only if a
        statistic is named, the measures launch only if a measure is named, and the entropy is computed only if named.  No
        host sync."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [k for k in names if k not in MICROSTRUCTURE_BC_NAMES]
        if unknown:
            raise ValueError(f"unknown behaviour characteristics {unknown}: the known names are "
                             f"{list(MICROSTRUCTURE_BC_NAMES)}")
        g = self._grids_arg(grids)
        stats = self.evaluate(g, region_cap=0)["stats"] if any(k in MICROSTRUCTURE_STAT_KEYS for k in names) else None
        meas = (self.measures(g, entropy="entropy" in names).bc
                if any(k in MICROSTRUCTURE_MEASURE_NAMES for k in names) else None)
        out = torch.zeros((g.shape[0], len(names)), dtype=torch.float64, device=self.device)
        for j, k in enumerate(names):
            if k in MICROSTRUCTURE_STAT_KEYS:
                out[:, j] = stats[:, MICROSTRUCTURE_STAT_KEYS.index(k)]
            elif k != "NONE":
                out[:, j] = meas[k]
        return out

    def close(self):
        self._closed = True
        self._entropy_tab = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
