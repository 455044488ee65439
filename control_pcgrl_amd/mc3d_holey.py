"""The 3-D holey dungeon and maze levels on the device: the statistics of Minecraft3DholeyDungeonProblem.get_stats
(probs/minecraft/minecraft_3D_holey_dungeon_prob.py:87-147) and Minecraft3DholeymazeProblem.get_stats
(probs/minecraft/minecraft_3D_holey_maze_prob.py:71-129), the loss ControlWrapper.get_loss would derive from them and the routes
behind them -- helper_3D.run_dijkstra under the player physics of helper_3D._passable: walk, step down, step up, a jump over a
one-tile gap -- for a batch of levels in one launch (include/pcgrl_amd_mc3d_holey.h, csrc/mc3d_holey/pcgrl_mc3d_holey.h,
DESIGN.md section 36).

This module evaluates levels; stepping holey environments (HoleyRepresentation, process_observation) is not built, nor the
2-D binary_holey, nor measures of 3-D maps.  The reference cannot construct either problem (Minecraft3DholeymazeProblem.__init__
calls Minecraft3DmazeProblem.__init__ without cfg), so the statistics and routes are pinned by levels recorded from instances
made with __new__, and the tables below by their restatement alone.  file:line references are relative to the reference's
control_pcgrl/envs/ directory.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .evaluator import EvaluatorCore
from .problems import ProblemSpec, fill_targets

MC3D_HOLEY_PROBLEMS = {"dungeon": 0, "maze": 1}
MC3D_HOLEY_TILES = {"dungeon": ["AIR", "DIRT", "CHEST", "SKULL", "PUMPKIN"], "maze": ["AIR", "DIRT"]}
MC3D_HOLEY_STAT_KEYS = {"dungeon": ["regions", "path-length", "chests", "enemies", "nearest-enemy", "n_jump"],  # dict order
                        "maze": ["regions", "path-length", "connected-path-length", "n_jump"]}
MC3D_HOLEY_PLAY_KEYS = ("searches", "accepted-1", "pushed-1", "accepted-2", "pushed-2", "x", "y", "z", "x2", "y2", "z2", "zero")
MC3D_HOLEY_MEASURE_NAMES = ("emptiness", "entropy", "symmetry", "symmetry-horizontal", "symmetry-vertical", "co-occurance")
ERR_TILE, ERR_HOLE, ERR_QUEUE = 1, 2, 4
MIN_AXIS, MAX_AXIS = 3, 16


def mc3d_holey_spec(problem="dungeon", map_shape=(7, 7, 7)) -> ProblemSpec:
    """The problem's tables.  minecraft_3D_maze_prob.py:33-35 sets _length = _width = _height = 15 before :46-58 derive the
    targets and bounds, so they are those of 15^3 whatever the map: _max_path_length = 2 * (15 // 3) *
    (ceil(15 / 2) * 15 + 15 // 2) = 1270.  The maze updates the plain maze's tables (minecraft_3D_holey_maze_prob.py:34-58),
    the dungeon replaces them (minecraft_3D_holey_dungeon_prob.py:30-84)."""
    if problem not in MC3D_HOLEY_PROBLEMS:
        raise ValueError(f"unknown problem {problem!r}: 'dungeon' or 'maze'")
    length = width = height = 15
    max_path = 2 * (height // 3) * (math.ceil(width / 2) * length + length // 2)
    regions_hi = math.ceil(width * length / 2 * height)
    if problem == "maze":
        trgs = {"regions": 1, "path-length": 10 * max_path, "connected-path-length": 10 * max_path, "n_jump": 5}
        bounds = {"regions": (0, regions_hi), "path-length": (0, max_path + 2), "connected-path-length": (0, max_path + 2),
                  "n_jump": (0, max_path // 2)}
        weights = {"regions": 0, "path-length": 100, "connected-path-length": 120, "n_jump": 150}
    else:
        any_tile = width * height * length // 4
        nearest = max_path // 2
        trgs = {"regions": 1, "path-length": 10 * max_path, "chests": 1, "enemies": (2, 5), "nearest-enemy": (5, nearest),
                "n_jump": (2, 5)}
        bounds = {"regions": (0, regions_hi), "path-length": (0, max_path), "chests": (0, any_tile), "enemies": (0, any_tile),
                  "nearest-enemy": (0, nearest), "n_jump": (0, max_path // 2)}
        weights = {"regions": 0, "path-length": 100, "chests": 300, "enemies": 100, "nearest-enemy": 200, "n_jump": 100}
    name = "minecraft_3D_dungeon_holey" if problem == "dungeon" else "minecraft_3D_holey_maze"
    return ProblemSpec(name, list(MC3D_HOLEY_TILES[problem]), list(MC3D_HOLEY_STAT_KEYS[problem]), trgs, bounds, dict(weights),
                       dict(weights))


def mc3d_holey_config(problem="dungeon", map_shape=(7, 7, 7), weights=None) -> "_lib.PcgrlMc3dHoleyConfig":
    """The C config of include/pcgrl_amd_mc3d_holey.h: the frozen targets as zero-loss intervals, and the weights."""
    spec = mc3d_holey_spec(problem, map_shape)
    cfg = _lib.PcgrlMc3dHoleyConfig()
    cfg.problem = MC3D_HOLEY_PROBLEMS[problem]
    cfg.z, cfg.y, cfg.x = (int(s) for s in map_shape)
    return fill_targets(cfg, spec, weights)


def hole_ok(foot, map_shape):
    """holey_prob_3D.py:28-31: the foot cell (z, y, x), bordered, is on one of the four side faces, off the edges, 1 <= z <= Z-1"""
    Z, Y, X = (int(s) for s in map_shape)
    z, y, x = (int(v) for v in foot)
    return 1 <= z <= Z - 1 and ((x in (0, X + 1) and 1 <= y <= Y) or (y in (0, Y + 1) and 1 <= x <= X))


def fixed_holes(map_shape=(7, 7, 7)):
    """The reference's fixed pair (holey_prob_3D.py:73-76): int32 [2, 3], the entrance foot (1, 0, X) and the exit foot
    (2, Y + 1, 1), (z, y, x) bordered"""
    Z, Y, X = (int(s) for s in map_shape)
    return np.array([[1, 0, X], [2, Y + 1, 1]], dtype=np.int32)


def all_holes(map_shape=(7, 7, 7)):
    """gen_all_holes' list (holey_prob_3D.py:35-39) as int32 [pairs, 2, 3] of foot cells, in its order: every ordered pair of
    border cells (get_border_idxs, argwhere order) whose exit foot is more than one cell away, along some axis, from the
    entrance's foot or head"""
    Z, Y, X = (int(s) for s in map_shape)
    d = np.zeros((Z + 2, Y + 2, X + 2), dtype=np.uint8)
    d[1:-2, 1:-1, 0] = 1
    d[1:-2, 1:-1, -1] = 1
    d[1:-2, 0, 1:-1] = 1
    d[1:-2, -1, 1:-1] = 1
    idx = np.argwhere(d == 1).astype(np.int32)
    a = np.repeat(idx, len(idx), axis=0)
    b = np.tile(idx, (len(idx), 1))
    head = a + np.array([1, 0, 0], dtype=np.int32)
    ok = np.maximum(np.abs(a - b).max(axis=1), np.abs(head - b).max(axis=1)) > 1
    return np.ascontiguousarray(np.stack([a[ok], b[ok]], axis=1))


class Mc3dHoleyEvaluator(EvaluatorCore):
    """Evaluates batches of 3-D holey dungeon or maze levels (interiors of 3..16 cells an axis) on one device.  Owns the search
    workspace, allocated once: one slot per workgroup of a launch (two rings of 8 bytes times the power of two >= 8 * bordered
    cells, and above 8^3 the per-cell search state: 128 KiB a slot at 7^3, 1.08 MiB at 15^3 and 16^3); `max_blocks` workgroups
    (None: 2048, fewer when that would pass 1 GiB) stride over the levels of a launch.  No host sync and no CPU fallback.
    Of the evaluators' shared code (evaluator.py) it has what needs no table: one launch covers a batch, there are three error
    bits and no measures."""

    RANK = 3

    def __init__(self, problem="dungeon", map_shape=(7, 7, 7), device="cuda:0", weights=None, max_blocks=None):
        if problem not in MC3D_HOLEY_PROBLEMS:
            raise ValueError(f"unknown problem {problem!r}: 'dungeon' or 'maze'")
        map_shape = self._map_shape_arg(map_shape, "the holey levels")
        self.problem, self.map_shape = problem, map_shape
        self.spec = mc3d_holey_spec(problem, map_shape)
        self.stat_keys = list(self.spec.stat_keys)
        slot = self._L.pcgrl_mc3d_holey_workspace_bytes(1, *map_shape)
        if slot < 0:
            raise NotImplementedError(f"mc3d_holey: map_shape {map_shape} outside {MIN_AXIS}..{MAX_AXIS} along an axis")
        if max_blocks is None:
            max_blocks = max(64, min(2048, (1 << 30) // slot))
        if int(max_blocks) < 1:
            raise ValueError("max_blocks must be at least 1")
        self.max_blocks = int(max_blocks)
        self._cfg = mc3d_holey_config(problem, map_shape, weights)
        self.weights = {k: self._cfg.weight[i] for i, k in enumerate(self.stat_keys)}
        self._open(device)
        self._workspace_bytes = slot * self.max_blocks
        self._workspace = torch.empty(self._workspace_bytes // 8, dtype=torch.int64, device=self.device)

    def _holes_arg(self, holes, n):
        h = torch.as_tensor(holes, device=self.device)
        if h.dtype != torch.int32:
            h = h.to(torch.int32)
        if h.dim() == 2:
            h = h.unsqueeze(0).expand(n, 2, 3)
        if tuple(h.shape) != (n, 2, 3):
            raise ValueError(f"holes must have shape [{n}, 2, 3] (or [2, 3] for all levels), got {list(h.shape)}")
        return h.contiguous()

    def evaluate(self, grids, holes, route_cap=0, overlay=False):
        """grids: uint8 [n][Z][Y][X] interiors (a device tensor at any alignment, or anything torch.as_tensor takes); holes:
        int32 [n][2][3], the entrance and exit foot cells (z, y, x) in bordered coordinates (one [2][3] pair serves all).
        Returns device tensors: stats int32 [n][6 or 4] (stat_keys order), loss float64 [n], error int32 [n] (ERR_TILE,
        ERR_HOLE, ERR_QUEUE), play int32 [n][12] (MC3D_HOLEY_PLAY_KEYS), route_len and route2_len int32 [n], leg_len int32
        [n][2]; with route_cap > 0 coords and coords2 int16 [n][route_cap][3] ((x, y, z), -1 past the end); with overlay
        overlay and overlay2 bool [n][Z+2][Y+2][X+2].  The header says which route is which."""
        g = self._levels_arg(grids)
        n = g.shape[0]
        h = self._holes_arg(holes, n)
        route_cap = int(route_cap)
        if route_cap < 0:
            raise ValueError("route_cap must not be negative")
        dev = self.device
        Z, Y, X = self.map_shape
        out = {"stats": torch.empty((n, len(self.stat_keys)), dtype=torch.int32, device=dev),
               "loss": torch.empty(n, dtype=torch.float64, device=dev),
               "play": torch.empty((n, 12), dtype=torch.int32, device=dev),
               "error": torch.empty(n, dtype=torch.int32, device=dev),
               "route_len": torch.empty(n, dtype=torch.int32, device=dev),
               "leg_len": torch.empty((n, 2), dtype=torch.int32, device=dev),
               "route2_len": torch.empty(n, dtype=torch.int32, device=dev)}
        if route_cap > 0:
            out["coords"] = torch.empty((n, route_cap, 3), dtype=torch.int16, device=dev)
            out["coords2"] = torch.empty((n, route_cap, 3), dtype=torch.int16, device=dev)
        if overlay:
            out["overlay"] = torch.empty((n, Z + 2, Y + 2, X + 2), dtype=torch.bool, device=dev)
            out["overlay2"] = torch.empty((n, Z + 2, Y + 2, X + 2), dtype=torch.bool, device=dev)

        def ptr(name):
            return out[name].data_ptr() if name in out else None

        with torch.cuda.device(dev):
            _lib.check(self._L.pcgrl_mc3d_holey_evaluate(
                C.byref(self._cfg), n, g.data_ptr(), h.data_ptr(), self._workspace.data_ptr(), self._workspace_bytes,
                route_cap, ptr("stats"), ptr("loss"), ptr("play"), ptr("error"), ptr("coords"), ptr("route_len"),
                ptr("leg_len"), ptr("coords2"), ptr("route2_len"), ptr("overlay"), ptr("overlay2"), self._stream()),
                "pcgrl_mc3d_holey_evaluate")
        for bit in (ERR_TILE, ERR_HOLE, ERR_QUEUE):  # the OR of the levels' bits, one bit at a time
            self._error |= (out["error"] & bit).max()
        return out

    def check_errors(self):
        """Raises if a launch of evaluate() since the last check read an unknown tile id (taken as DIRT) or filled a search's
        ring; a refused hole is a level's own answer (error bit ERR_HOLE) and does not raise.  Synchronises."""
        bits = int(self._error.item())
        self._error.zero_()
        if bits & ERR_TILE:
            raise ValueError(f"mc3d_holey: a tile id the {self.problem} does not know was seen on the device (read as DIRT)")
        if bits & ERR_QUEUE:
            raise RuntimeError("mc3d_holey: a search filled its ring (see include/pcgrl_amd_mc3d_holey.h); the level has no answer")

    def check_names(self, names):
        """what behaviour() takes: the problem's statistic names and "NONE" """
        for k in names:
            if k in MC3D_HOLEY_MEASURE_NAMES:
                raise NotImplementedError(f"mc3d_holey: the measure {k!r} is not built for 3-D maps: the shared measures wave "
                                          "body is 2-D")
            if k not in self.stat_keys and k != "NONE":
                raise ValueError(f"unknown behaviour characteristic {k!r}: the known names are {self.stat_keys + ['NONE']}")

    def behaviour(self, grids, holes, names):
        """The behaviour vector of each level: float64 [n, len(names)], column j the reference's get_bc(names[j], ...)
        (evo/evolve.py:606-635): a statistic's name is that column of evaluate()'s stats, "NONE" is 0.  The measure names are
        refused: the shared measures wave body is 2-D.  No host sync."""
        names = [names] if isinstance(names, str) else list(names)
        self.check_names(names)
        g = self._grids_arg(grids)
        stats = self.evaluate(g, holes)["stats"] if any(k != "NONE" for k in names) else None
        out = torch.zeros((g.shape[0], len(names)), dtype=torch.float64, device=self.device)
        for j, k in enumerate(names):
            if k != "NONE":
                out[:, j] = stats[:, self.stat_keys.index(k)]
        return out
