"""MiniDungeon levels on the device: the eleven statistics of MDungeonProblem.get_stats (probs/mdungeon/mdungeon_prob.py:151-171)
-- six counts and scans of the map and, for a level with one player, one exit and one region, the four-stage play-through of
probs/mdungeon/mdungeon/engine.py (A* at balance 1, 0.5 and 0, then BFS) -- for a batch of maps in one launch, the returned
node's move list, the reward and the episode end of the problem, and the level measures, the pairwise Hamming diversity and the
behaviour vector the reference's quality-diversity loop places a level by (include/pcgrl_amd_mdungeon.h,
csrc/mdungeon/pcgrl_mdungeon.h).  What it shares with Dangerous Dave is in playthrough.py.

This module evaluates and measures maps; stepping MiniDungeon environments is not built (the reference cannot construct the
problem, so no episode could be recorded to pin one against).  It is not part of the 2-D engine, so PROBLEMS / problem_spec /
build_config / make_vec_env do not know "mdungeon".  file:line references are relative to the reference's control_pcgrl/envs/
directory.
"""
import math

import torch

from . import _lib
from .playthrough import MAX_H, MAX_W, MAX_SOLVER_POWER, PlaythroughEvaluator  # noqa: F401 (this module's names)
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
MAX_ITEMS = 64


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


class MDungeonEvaluator(PlaythroughEvaluator):
    """Evaluates batches of MiniDungeon maps (1..16 rows x 1..32 columns) on one device.  Owns the search workspace: per level
    20 * (4 * solver_power + 1) bytes of nodes and open list and 12 bytes for each of the C >= 2 * solver_power slots of the
    visited set -- 596 640 bytes at the stock power of 5 000 (C = 16 384), 2.4 GB for max_levels = 4 096.
    Batches above max_levels run as successive launches on the current stream.  No host sync and no CPU fallback.

    evaluate()'s stats are in MDUNGEON_STAT_KEYS order and its play columns are MDUNGEON_PLAY_KEYS: the status (5: more than
    64 items), the four stages' iterations, the returned node's x, y, health, col_potions, col_treasures, col_enemies and
    depth; moves are indices into MDUNGEON_MOVES.  A tile id above 7 reads as solid and sets the error.  reward() is
    MDungeonProblem.get_reward (mdungeon_prob.py:183-205), measures() counts T = 8 tiles."""

    NAME, TILES, STAT_KEYS, REWARD_ORDER = "mdungeon", MDUNGEON_TILES, MDUNGEON_STAT_KEYS, MDUNGEON_REWARD_ORDER
    MEASURE_NAMES, BC_NAMES = MDUNGEON_MEASURE_NAMES, MDUNGEON_BC_NAMES

    def __init__(self, map_shape=(11, 7), device="cuda:0", solver_power=5000, weights=None, max_enemies=6, max_potions=2,
                 max_treasures=3, target_col_enemies=0.5, target_solution=20, max_levels=4096):
        self.max_enemies, self.max_potions, self.max_treasures = int(max_enemies), int(max_potions), int(max_treasures)
        self.target_col_enemies, self.target_solution = float(target_col_enemies), int(target_solution)
        super().__init__(map_shape, device, solver_power, max_levels, mdungeon_spec,
                         lambda shape, power: mdungeon_config(shape, power, weights, max_enemies, max_potions, max_treasures,
                                                              target_col_enemies, target_solution))

    def _bounds(self):
        """get_reward's ranges (mdungeon_prob.py:185-195)"""
        inf = math.inf
        return {"player": (1, 1), "exit": (1, 1), "potions": (-inf, self.max_potions), "treasures": (-inf, self.max_treasures),
                "enemies": (1, self.max_enemies), "regions": (1, 1), "col-enemies": (inf, inf), "dist-win": (-inf, -inf),
                "sol-length": (inf, inf)}

    def episode_over(self, stats):
        """MDungeonProblem.get_episode_over (mdungeon_prob.py:218-221): bool [n]; the share of enemies met is a float64
        division, as the reference's"""
        s = self._stats_arg(stats)
        enemies = s[:, 4]
        share = s[:, 8].to(torch.float64) / torch.clamp(enemies, min=1).to(torch.float64)
        return (s[:, 10] >= self.target_solution) & (enemies > 0) & (share > self.target_col_enemies)
