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
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .measures import MeasuresMixin
from .problems import ProblemSpec, target_interval

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
    spec = loderunner_spec(map_shape)
    weights = dict(spec.default_weights) if weights is None else dict(weights)
    unknown = set(weights) - set(spec.stat_keys)
    if unknown:
        raise ValueError(f"unknown loderunner statistics in weights: {sorted(unknown)}")
    cfg = _lib.PcgrlLoderunnerConfig()
    cfg.h, cfg.w = int(map_shape[0]), int(map_shape[1])
    for i, k in enumerate(spec.stat_keys):
        lo, hi = target_interval(spec.static_trgs[k])
        cfg.has_trg[i] = 1
        cfg.weight[i] = float(weights.get(k, 0.0))
        cfg.trg_lo[i], cfg.trg_hi[i] = lo, hi
    return cfg


class LodeRunnerEvaluator(MeasuresMixin):
    """Evaluates batches of Lode Runner maps on one device.  Owns the search workspace, a torch tensor sized at the first
    evaluate() for the launch it needs (pcgrl_loderunner_workspace_bytes(min(n, max_levels), H, W) bytes: one slot per block of
    the launch -- 150 KiB per level at 8 x 12 up to 4096 levels, 598 MiB; never more than 640 MiB) and grown when a larger batch
    comes; batches above max_levels run as successive launches on the current stream.  A call to be captured in a graph wants
    one eager call of the same size before it, so that the capture allocates no workspace.  There is no wall-clock limit
    (see the module docstring) and no CPU fallback."""

    def __init__(self, map_shape=(8, 12), device="cuda:0", weights=None, max_levels=4096):
        self._L = _lib.lib()
        map_shape = tuple(int(s) for s in map_shape)
        if len(map_shape) != 2:
            raise ValueError(f"loderunner maps are 2-D, got shape {map_shape}")
        if int(max_levels) < 1:
            raise ValueError("max_levels must be at least 1")
        self.map_shape = map_shape
        self.spec = loderunner_spec(map_shape)
        self.max_levels = int(max_levels)
        self._cfg = loderunner_config(map_shape, weights)
        nbytes = self._L.pcgrl_loderunner_workspace_bytes(self.max_levels, map_shape[0], map_shape[1])
        if nbytes < 0:
            raise NotImplementedError(f"loderunner: map_shape {map_shape} outside 1..{MAX_H} x 1..{MAX_W}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("LodeRunnerEvaluator needs a cuda device: there is no CPU fallback")
        self._workspace, self._workspace_bytes, self._closed = None, 0, False  # sized by the first evaluate()
        self._error = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _grow_workspace(self, n):
        """the workspace a launch over min(n, max_levels) levels needs (inside torch.cuda.device(self.device))"""
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
        if self._closed:
            raise RuntimeError("LodeRunnerEvaluator is closed")
        g = torch.as_tensor(grids, device=self.device)
        if g.dtype != torch.uint8:
            g = g.to(torch.uint8)
        if g.dim() == 2:
            g = g.unsqueeze(0)
        if g.dim() != 3 or tuple(g.shape[1:]) != self.map_shape:
            raise ValueError(f"grids must have shape [n]{list(self.map_shape)}, got {list(g.shape)}")
        g = g.contiguous()
        n = g.shape[0]
        if n < 1:
            raise ValueError("no levels to evaluate")
        gold_cap = int(gold_cap)
        if gold_cap < 0:
            raise ValueError("gold_cap must not be negative")
        dev = self.device
        out = {"stats": torch.empty((n, 5), dtype=torch.float64, device=dev),
               "loss": torch.empty(n, dtype=torch.float64, device=dev),
               "play": torch.empty((n, 4), dtype=torch.int32, device=dev)}
        if gold_cap > 0:
            out["gold_state"] = torch.empty((n, gold_cap), dtype=torch.int8, device=dev)
            out["gold_dist"] = torch.empty((n, gold_cap), dtype=torch.int16, device=dev)
        err = torch.empty(n, dtype=torch.int32, device=dev)

        def ptr(name, lo):
            return out[name][lo:].data_ptr() if name in out else None

        with torch.cuda.device(dev):
            stream = self._stream()
            self._grow_workspace(n)
            for lo in range(0, n, self.max_levels):
                m = min(self.max_levels, n - lo)
                _lib.check(self._L.pcgrl_loderunner_evaluate(
                    C.byref(self._cfg), m, g[lo:].data_ptr(), self._workspace.data_ptr(), self._workspace_bytes, gold_cap,
                    ptr("stats", lo), ptr("loss", lo), ptr("play", lo), ptr("gold_state", lo), ptr("gold_dist", lo),
                    err[lo:].data_ptr(), stream), "pcgrl_loderunner_evaluate")
        self._error |= err.max()
        out["error"] = err
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
        g = self._grids_arg(grids)
        n = g.shape[0]
        if n < 1:
            raise ValueError("no levels to evaluate")
        gold_cap = int(gold_cap)
        if gold_cap < 0:
            raise ValueError("gold_cap must not be negative")
        route_cap = 8 * self.map_shape[0] * self.map_shape[1] if route_cap is None else int(route_cap)
        if route_cap < 0:
            raise ValueError("route_cap must not be negative")
        dev = self.device
        out = {"stats": torch.empty((n, 5), dtype=torch.float64, device=dev),
               "loss": torch.empty(n, dtype=torch.float64, device=dev),
               "play": torch.empty((n, 4), dtype=torch.int32, device=dev),
               "tour_len": torch.empty(n, dtype=torch.int32, device=dev),
               "coords": torch.empty((n, route_cap, 2), dtype=torch.int16, device=dev)}
        if moves:
            out["moves"] = torch.empty((n, route_cap), dtype=torch.int8, device=dev)
        if gold_cap > 0:
            out["gold_state"] = torch.empty((n, gold_cap), dtype=torch.int8, device=dev)
            out["gold_dist"] = torch.empty((n, gold_cap), dtype=torch.int16, device=dev)
            out["gold_off"] = torch.empty((n, gold_cap), dtype=torch.int32, device=dev)
            out["gold_back"] = torch.empty((n, gold_cap), dtype=torch.int16, device=dev)
        err = torch.empty(n, dtype=torch.int32, device=dev)

        def ptr(name, lo):
            return out[name][lo:].data_ptr() if name in out and out[name].numel() else None

        with torch.cuda.device(dev):
            stream = self._stream()
            self._grow_workspace(n)
            for lo in range(0, n, self.max_levels):
                m = min(self.max_levels, n - lo)
                _lib.check(self._L.pcgrl_loderunner_routes(
                    C.byref(self._cfg), m, g[lo:].data_ptr(), self._workspace.data_ptr(), self._workspace_bytes, gold_cap,
                    route_cap, ptr("stats", lo), ptr("loss", lo), ptr("play", lo), ptr("gold_state", lo), ptr("gold_dist", lo),
                    ptr("gold_off", lo), ptr("gold_back", lo), ptr("coords", lo), ptr("moves", lo), ptr("tour_len", lo),
                    err[lo:].data_ptr(), stream), "pcgrl_loderunner_routes")
        self._error |= err.max()
        out["error"] = err
        out["win"] = out["stats"][:, 3]
        out["path_length"] = out["stats"][:, 4]
        return out

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

    def check_errors(self):
        """Raises if a launch of evaluate() or routes() since the last check read a tile id above 7 (it was taken as empty).  Synchronises.
        measures() / diversity() mask ids to 3 bits and set no error."""
        bits = int(self._error.item())
        self._error.zero_()
        if bits & 1:
            raise ValueError("loderunner: a tile id above 7 was seen on the device (read as empty)")

    def _meas_dims(self):
        return self.map_shape[0] * self.map_shape[1], len(LODERUNNER_TILES)

    def _grids_arg(self, grids):
        if self._closed:
            raise RuntimeError("LodeRunnerEvaluator is closed")
        g = torch.as_tensor(grids, device=self.device)
        if g.dtype != torch.uint8:
            g = g.to(torch.uint8)
        if g.dim() == 2:
            g = g.unsqueeze(0)
        if g.dim() != 3 or tuple(g.shape[1:]) != self.map_shape:
            raise ValueError(f"grids must have shape [n]{list(self.map_shape)}, got {list(g.shape)}")
        return g.contiguous()

    def measures(self, grids, entropy=True):
        """The behaviour characteristics of the maps that the reference computes from the integer map (evo/evolve.py:606-635
        get_bc -> :423-592), as SmbEvaluator.measures returns them with T = 8: counts int32 [n, 8], match int32 [n, 3]
        (horizontal, vertical, wrapped co-occurance matches), forms float64 [n, 13], tile_fractions float64 [n, 8] and bc, a
        dict under get_bc's names -> float64 [n] (also .entropy, .emptiness).  All but entropy equal the reference bit for bit;
        entropy does on the host whose numpy built the table.  The divisors are the map's own H * W.  grids: uint8 [n][H][W] at
        any alignment, n >= 0; ids are masked to 3 bits and set no error.  One launch on the current stream, no host sync."""
        g = self._grids_arg(grids)
        H, W, n = *self.map_shape, g.shape[0]
        return self._measures_result(self._L.pcgrl_loderunner_measures_for_grids, (H, W, n, g.data_ptr()), n, entropy)

    def diversity(self, grids, group=None, pairwise=False):
        """Pairwise Hamming distances (cells whose tiles differ) among the maps in consecutive groups of `group` maps (None: one
        group of all), as SmbEvaluator.diversity returns them: hamming_sum int64 [G], scores float64 [G, 2], nearest /
        nearest_idx int32 [n] (the lowest index on ties), div_score (rl/evaluate_ctrl.py:42-48) and diversity_bonus
        (evo/evolve.py:1236-1244) float64 [G], pairwise int32 [G, K, K] or None.  Three launches on the current stream, no host
        sync."""
        g = self._grids_arg(grids)
        H, W, n = *self.map_shape, g.shape[0]
        return self._diversity_result(self._L.pcgrl_loderunner_diversity_for_grids, (H, W, n, g.data_ptr()), n, group, pairwise,
                                      self._L.pcgrl_loderunner_diversity_scratch_bytes(H, W, n))

    def behaviour(self, grids, names):
        """The behaviour vector of each map: float64 [n, len(names)], column j the reference's get_bc(names[j], ...)
        (evo/evolve.py:606-635).  A name among spec.stat_keys is that column of evaluate()'s stats (get_bc looks there first); a
        name of LODERUNNER_MEASURE_NAMES is the measure of that name; "NONE" is 0.  evaluate(gold_cap=0) runs only if a
        statistic is named, the measures launch only if a measure is named, and the entropy is computed only if named.  No host
        sync.  The quality-diversity loop's pairs for this problem (configs/evo/batch.yaml) are ("emptiness", "path-length") and
        ("symmetry", "path-length")."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [k for k in names if k not in LODERUNNER_BC_NAMES]
        if unknown:
            raise ValueError(f"unknown behaviour characteristics {unknown}: the known names are {list(LODERUNNER_BC_NAMES)}")
        g = self._grids_arg(grids)
        stats = self.evaluate(g, gold_cap=0)["stats"] if any(k in LODERUNNER_STAT_KEYS for k in names) else None
        meas = (self.measures(g, entropy="entropy" in names).bc
                if any(k in LODERUNNER_MEASURE_NAMES for k in names) else None)
        out = torch.zeros((g.shape[0], len(names)), dtype=torch.float64, device=self.device)
        for j, k in enumerate(names):
            if k in LODERUNNER_STAT_KEYS:
                out[:, j] = stats[:, LODERUNNER_STAT_KEYS.index(k)]
            elif k != "NONE":
                out[:, j] = meas[k]
        return out

    def close(self):
        self._workspace, self._workspace_bytes, self._closed = None, 0, True
        self._entropy_tab = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
