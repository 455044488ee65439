"""Lode Runner levels on the device: the five statistics of LoderunnerProblem.get_stats, the loss ControlWrapper.get_loss
would derive from them and the per-gold record of the gold searches behind `win` and `path-length`, for a batch of maps in one
launch (include/pcgrl_amd_loderunner.h, csrc/loderunner/pcgrl_loderunner.h); and the level measures,
the pairwise Hamming diversity and the behaviour vector the reference's quality-diversity loop places a level by
(include/pcgrl_amd_loderunner_measures.h, csrc/loderunner/pcgrl_loderunner_measures.h); and the routes
behind `path-length`, the cells of both A* paths of every gold collected by its own searches
(include/pcgrl_amd_loderunner_routes.h, csrc/loderunner/pcgrl_loderunner_routes.h).

This module evaluates and measures maps and lists their routes; stepping Lode Runner environments is not built.  It is not part of the 2-D engine, so PROBLEMS /
problem_spec / build_config do not know "loderunner".  file:line references are relative to the reference's
control_pcgrl/envs/probs/ directory.

The reference abandons an evaluation after one second of wall clock (loderunner/engine.py:254, 287, 293).  The device has no
such limit: its result is the reference's with the clock stopped.  At the stock 8 x 12 the limit does not bite; above the stock
size the reference's own answer depends on the host's speed.
"""
import math

import numpy as np
import torch

from . import _lib
from .evaluator import LevelEvaluator
from .problems import ProblemSpec, fill_targets

LODERUNNER_TILES = ["empty", "brick", "ladder", "rope", "solid", "gold", "enemy", "player"]  # loderunner_prob.py:46
LODERUNNER_STAT_KEYS = ["player", "enemies", "gold", "win", "path-length"]
LODERUNNER_MEASURE_NAMES = ("emptiness", "entropy", "symmetry", "symmetry-horizontal", "symmetry-vertical", "co-occurance")
# what behaviour() takes: get_bc (evo/evolve.py:606-635) looks in the statistics first, then among the measures of the map
LODERUNNER_BC_NAMES = tuple(LODERUNNER_STAT_KEYS) + LODERUNNER_MEASURE_NAMES + ("NONE",)
MAX_H, MAX_W = 16, 32


def loderunner_spec(map_shape=(8, 12)) -> ProblemSpec:
    """loderunner_prob.py:13-14 sets _width = 12, _height = 8 BEFORE loderunner_ctrl_prob.py:20-44 derive the path-length
    target and the bounds, so those are frozen at the stock size whatever the map."""
    fw, fh = 12, 8
    n = fw * fh
    max_path = float((math.ceil(fw / 2) * fh + math.floor(fh / 2)) * 2 - 1)  # 103.0
    weights = {"player": 1, "enemies": 0, "gold": 0, "win": 1, "path-length": 0}  # loderunner_prob.py:35-44 _reward_weights
    return ProblemSpec(
        "loderunner", list(LODERUNNER_TILES), list(LODERUNNER_STAT_KEYS),
        {"player": 1, "enemies": 2, "gold": (1, 10), "win": 1, "path-length": max_path},
        {"player": (0, n), "enemies": (0, n), "gold": (0, 10), "win": (0, 1), "path-length": (0, max_path)},
        dict(weights), dict(weights),
    )


def loderunner_config(map_shape=(8, 12), weights=None) -> "_lib.PcgrlLoderunnerConfig":
    """The C config of include/pcgrl_amd_loderunner.h: the frozen targets as zero-loss intervals, and the weights."""
    cfg = _lib.PcgrlLoderunnerConfig()
    cfg.h, cfg.w = int(map_shape[0]), int(map_shape[1])
    return fill_targets(cfg, loderunner_spec(map_shape), weights, "loderunner statistics")


class LodeRunnerEvaluator(LevelEvaluator):
    """Evaluates batches of Lode Runner maps on one device.  Owns the search workspace, a torch tensor sized at the first
    evaluate() for the launch it needs (pcgrl_loderunner_workspace_bytes(min(n, max_levels), H, W) bytes: one slot per block of
    the launch -- 150 KiB per level at 8 x 12 up to 4096 levels, 598 MiB; never more than 640 MiB) and grown when a larger batch
    comes; batches above max_levels run as successive launches on the current stream.  A call to be captured in a graph wants
    one eager call of the same size before it, so that the capture allocates no workspace.  There is no wall-clock limit
    (see the module docstring) and no CPU fallback.

    A tile id above 7 reads as empty and sets the error of evaluate() and routes().  measures() counts T = 8 tiles (forms
    float64 [n, 13]); the quality-diversity loop's pairs for behaviour() (configs/evo/batch.yaml) are ("emptiness",
    "path-length") and ("symmetry", "path-length")."""

    NAME, TILES, STAT_KEYS, TILE_READ_AS = "loderunner", LODERUNNER_TILES, LODERUNNER_STAT_KEYS, "empty"
    MEASURE_NAMES, BC_NAMES, STATS_ONLY = LODERUNNER_MEASURE_NAMES, LODERUNNER_BC_NAMES, "gold_cap"
    # the outputs of pcgrl_loderunner_routes in its order; pcgrl_loderunner_evaluate has the first five
    _OUTPUTS = ("stats", "loss", "play", "gold_state", "gold_dist", "gold_off", "gold_back", "coords", "moves", "tour_len")

    def __init__(self, map_shape=(8, 12), device="cuda:0", weights=None, max_levels=4096):
        super().__init__(map_shape, max_levels)
        map_shape = self.map_shape
        self.spec = loderunner_spec(map_shape)
        self._cfg = loderunner_config(map_shape, weights)
        nbytes = self._L.pcgrl_loderunner_workspace_bytes(self.max_levels, map_shape[0], map_shape[1])
        if nbytes < 0:
            raise NotImplementedError(f"loderunner: map_shape {map_shape} outside 1..{MAX_H} x 1..{MAX_W}")
        self._open(device)
        self._workspace_bytes = 0  # the workspace is sized by the first evaluate()

    def _grow_workspace(self, n):
        """the workspace a launch over min(n, max_levels) levels needs"""
        need = self._L.pcgrl_loderunner_workspace_bytes(min(n, self.max_levels), self.map_shape[0], self.map_shape[1])
        if need > self._workspace_bytes:
            if self._workspace is not None:  # launches already enqueued on this stream keep it until they are done
                self._workspace.record_stream(torch.cuda.current_stream(self.device))
            self._workspace = torch.empty(need // 4, dtype=torch.int32, device=self.device)
            self._workspace_bytes = need

    def evaluate(self, grids, gold_cap=32):
        """grids: uint8 [n][H][W] (a device tensor, or anything torch.as_tensor takes).  Returns device tensors: stats float64
        [n][5] (spec.stat_keys order; win and path_length are views of its columns), loss float64 [n], play int32 [n][4]
        (searched, landing row, landing column, golds collected including those on the starting fall), and with gold_cap > 0:
        gold_state int8 [n][gold_cap] (per gold in row-major order 0 not collected, 1 by its own pair of searches, 2 on
        another gold's path, 3 on the starting fall, -1 past the last gold) and gold_dist int16 [n][gold_cap] (what the gold
        added to path-length).  The totals stay complete when gold_cap is smaller than the number of golds."""
        g, gold_cap, out = self._begin(grids, gold_cap)
        return self._finish(self._call("evaluate"), g, (gold_cap,), out, self._OUTPUTS[:5])

    def _begin(self, grids, gold_cap):
        """the checks and the outputs that evaluate() and routes() share"""
        g = self._levels_arg(grids)
        n, dev = g.shape[0], self.device
        gold_cap = int(gold_cap)
        if gold_cap < 0:
            raise ValueError("gold_cap must not be negative")
        out = {"stats": torch.empty((n, 5), dtype=torch.float64, device=dev),
               "loss": torch.empty(n, dtype=torch.float64, device=dev),
               "play": torch.empty((n, 4), dtype=torch.int32, device=dev)}
        if gold_cap > 0:
            out["gold_state"] = torch.empty((n, gold_cap), dtype=torch.int8, device=dev)
            out["gold_dist"] = torch.empty((n, gold_cap), dtype=torch.int16, device=dev)
        return g, gold_cap, out

    def _finish(self, fn, g, caps, out, names):
        self._grow_workspace(g.shape[0])
        out["error"] = self._launch(fn, g, (self._workspace.data_ptr(), self._workspace_bytes, *caps), out, names)
        out["win"] = out["stats"][:, 3]
        out["path_length"] = out["stats"][:, 4]
        return out

    def routes(self, grids, gold_cap=32, route_cap=None, moves=False):
        """evaluate() and the routes behind path-length, in one launch per max_levels levels (no second search: the kernel of
        evaluate() with the parent chains read out).  Returns evaluate()'s dict and, as device tensors,
          tour_len   int32 [n]: the cells of the level's tour -- for each gold in state 1, in gold order, its outward route
                     (landing cell ... gold, gold_dist cells: reversed(to_goal.get_path()[0]) of the reference's
                     find_all_golds) then its return route (gold ... landing cell, gold_back cells)
          coords     int16 [n][route_cap][2]: the tour as (row, column), (-1, -1) past its end
          moves      int8 [n][route_cap], if asked: entry k the move from coords[k] to coords[k + 1] (0..5 = left right up down
                     d-left d-right, the reference's Node.action); -1 at the last cell of each route and past the end
          gold_off   int32 [n][gold_cap]: where the gold's outward route starts in the tour (its return route at
                     off + gold_dist); -1 unless the state is 1
          gold_back  int16 [n][gold_cap]: the cells of the return route; 0 unless the state is 1
        (gold_off / gold_back with gold_cap > 0).  route_cap=None is 8 * H * W; route_cap=0 stores no cells, and since tour_len
        and gold_off stay complete whatever the caps cut, it sizes a second call.  split_routes() cuts a level's tour up."""
        g, gold_cap, out = self._begin(grids, gold_cap)
        n, dev = g.shape[0], self.device
        route_cap = 8 * self.map_shape[0] * self.map_shape[1] if route_cap is None else int(route_cap)
        if route_cap < 0:
            raise ValueError("route_cap must not be negative")
        out["tour_len"] = torch.empty(n, dtype=torch.int32, device=dev)
        out["coords"] = torch.empty((n, route_cap, 2), dtype=torch.int16, device=dev)
        if moves:
            out["moves"] = torch.empty((n, route_cap), dtype=torch.int8, device=dev)
        if gold_cap > 0:
            out["gold_off"] = torch.empty((n, gold_cap), dtype=torch.int32, device=dev)
            out["gold_back"] = torch.empty((n, gold_cap), dtype=torch.int16, device=dev)
        return self._finish(self._call("routes"), g, (gold_cap, route_cap), out, self._OUTPUTS)

    @staticmethod
    def split_routes(result, i):
        """Level i of a routes() result cut up on the host: a list of (gold_cell, outward, back), one entry per gold in state
        1 in gold order, each route a list of (row, column) -- outward from the landing cell to gold_cell, back from gold_cell
        to the landing cell.  Needs gold_off (gold_cap > 0); raises if gold_cap or route_cap cut a route of the level.
        Synchronises (it copies the level's rows to the host)."""
        if "gold_off" not in result:
            raise ValueError("split_routes needs a routes() result with gold_cap > 0")
        state = np.asarray(torch.as_tensor(result["gold_state"][i]).cpu())
        dist = np.asarray(torch.as_tensor(result["gold_dist"][i]).cpu())
        off = np.asarray(torch.as_tensor(result["gold_off"][i]).cpu())
        back = np.asarray(torch.as_tensor(result["gold_back"][i]).cpu())
        coords = np.asarray(torch.as_tensor(result["coords"][i]).cpu())
        tour = int(torch.as_tensor(result["tour_len"][i]).item())
        if tour > len(coords):
            raise ValueError(f"level {i}: the tour has {tour} cells, route_cap kept {len(coords)}")
        out, seen = [], 0
        for j in np.flatnonzero(state == 1):
            o, d, b = int(off[j]), int(dist[j]), int(back[j])
            outward = [(int(r), int(c)) for r, c in coords[o:o + d]]
            out.append((outward[-1], outward, [(int(r), int(c)) for r, c in coords[o + d:o + d + b]]))
            seen += d + b
        if seen != tour:
            raise ValueError(f"level {i}: gold_cap cut the per-gold record ({seen} of {tour} cells are accounted for)")
        return out
