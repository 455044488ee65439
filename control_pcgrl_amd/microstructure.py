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
import math

import torch

from . import _lib
from .evaluator import LevelEvaluator
from .problems import ProblemSpec, fill_targets

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
    cfg = _lib.PcgrlMicrostructureConfig()
    cfg.h, cfg.w = int(map_shape[0]), int(map_shape[1])
    return fill_targets(cfg, microstructure_spec(map_shape), weights, "microstructure statistics")


class MicrostructureEvaluator(LevelEvaluator):
    """Evaluates batches of microstructure maps (1..64 rows x 1..64 columns) on one device.  The kernel needs no workspace;
    batches above max_levels run as successive launches on the current stream.  No host sync and no CPU fallback.  A tile id
    above 1 reads as solid and sets the error of evaluate(); measures() counts T = 2 tiles (forms float64 [n, 7])."""

    NAME, TILES, STAT_KEYS, TILE_READ_AS = "microstructure", MICROSTRUCTURE_TILES, MICROSTRUCTURE_STAT_KEYS, "solid"
    MEASURE_NAMES, BC_NAMES, STATS_ONLY = MICROSTRUCTURE_MEASURE_NAMES, MICROSTRUCTURE_BC_NAMES, "region_cap"

    def __init__(self, map_shape=(64, 64), device="cuda:0", weights=None, max_levels=4096):
        super().__init__(map_shape, max_levels)
        map_shape = self.map_shape
        self.spec = microstructure_spec(map_shape)
        self._cfg = microstructure_config(map_shape, weights)
        if not (1 <= map_shape[0] <= MAX_H and 1 <= map_shape[1] <= MAX_W):
            raise NotImplementedError(f"microstructure: map_shape {map_shape} outside 1..{MAX_H} x 1..{MAX_W}")
        self._open(device)

    def evaluate(self, grids, region_cap=0):
        """grids: uint8 [n][H][W] (a device tensor at any alignment, or anything torch.as_tensor takes).  Returns device
        tensors: stats float64 [n][2] (spec.stat_keys order; path_length and tortuosity are views of its columns), loss float64
        [n], regions int32 [n] (the number of regions, the mean's divisor), error int32 [n], and with region_cap > 0:
        region_rec int16 [n][region_cap][5] (per region in visit order start row, start column, far row, far column, d; -1
        past the last region) and region_tort float64 [n][region_cap] (0 past it).  The totals stay complete when region_cap
        is smaller than the number of regions."""
        g = self._levels_arg(grids)
        n, dev = g.shape[0], self.device
        region_cap = int(region_cap)
        if region_cap < 0:
            raise ValueError("region_cap must not be negative")
        out = {"stats": torch.empty((n, 2), dtype=torch.float64, device=dev),
               "loss": torch.empty(n, dtype=torch.float64, device=dev),
               "regions": torch.empty(n, dtype=torch.int32, device=dev)}
        if region_cap > 0:
            out["region_rec"] = torch.empty((n, region_cap, 5), dtype=torch.int16, device=dev)
            out["region_tort"] = torch.empty((n, region_cap), dtype=torch.float64, device=dev)
        out["error"] = self._launch(self._call("evaluate"), g, (region_cap,), out,
                                    ("stats", "loss", "regions", "region_rec", "region_tort"))
        out["path_length"] = out["stats"][:, 0]
        out["tortuosity"] = out["stats"][:, 1]
        return out
