"""Dangerous Dave levels on the device: the eleven statistics of DDaveProblem.get_stats (probs/ddave/ddave_prob.py:149-169) --
seven counts and scans of the map and, for a level with one player, one exit, one key and one region, the four-stage
play-through of probs/ddave/ddave/engine.py (A* at balance 1, 0.5 and 0, then BFS) -- for a batch of maps in one launch, the
returned node's action list, the reward and the episode end of the problem, and the level measures, the pairwise Hamming
diversity and the behaviour vector the reference's quality-diversity loop places a level by (include/pcgrl_amd_ddave.h,
csrc/ddave/pcgrl_ddave.h).  What it shares with MiniDungeon is in playthrough.py.

This module evaluates and measures maps; stepping Dangerous Dave environments is not built (the reference cannot construct the
problem, so no episode could be recorded to pin one against).  It is not part of the 2-D engine, so PROBLEMS / problem_spec /
build_config / make_vec_env do not know "ddave".  file:line references are relative to the reference's control_pcgrl/envs/
directory.
"""
import math

from . import _lib
from .playthrough import MAX_H, MAX_W, MAX_SOLVER_POWER, PlaythroughEvaluator, _range_reward  # noqa: F401 (this module's names)
from .problems import ProblemSpec

DDAVE_TILES = ["empty", "solid", "player", "exit", "diamond", "key", "spike"]  # ddave_prob.py:53-54
DDAVE_STAT_KEYS = ["player", "dist-floor", "exit", "diamonds", "key", "spikes", "regions", "num-jumps", "col-diamonds",
                   "dist-win", "sol-length"]  # get_stats' dict order, ddave_prob.py:151-163
DDAVE_MOVES = ((0, 0), (-1, 0), (1, 0), (0, -1))  # engine.py:3 directions as (x, y): stay, left, right, jump
# get_reward's order of summation (ddave_prob.py:196-205); col-diamonds has no term
DDAVE_REWARD_ORDER = ("player", "dist-floor", "exit", "spikes", "diamonds", "key", "regions", "num-jumps", "dist-win",
                      "sol-length")
DDAVE_WEIGHTS = {"player": 3, "dist-floor": 2, "exit": 3, "diamonds": 1, "key": 3, "spikes": 1, "regions": 5, "num-jumps": 3,
                 "dist-win": 0.1, "sol-length": 1}  # ddave_prob.py:31-42
DDAVE_PLAY_KEYS = ("status", "iterations-1", "iterations-2", "iterations-3", "iterations-4", "x", "y", "airTime", "health",
                   "col_key", "diamonds", "depth")
DDAVE_MEASURE_NAMES = ("emptiness", "entropy", "symmetry", "symmetry-horizontal", "symmetry-vertical", "co-occurance")
# what behaviour() takes: get_bc (evo/evolve.py:606-635) looks in the statistics first, then among the measures of the map
DDAVE_BC_NAMES = tuple(DDAVE_STAT_KEYS) + DDAVE_MEASURE_NAMES + ("NONE",)
MAX_DIAMONDS = 64


def ddave_spec(map_shape=(7, 11)) -> ProblemSpec:
    """The problem's tables.  DDaveProblem has no static targets and no conditional bounds of its own (it predates the
    control wrapper): the reward's ranges live in get_reward (ddave_prob.py:184-193) and DDaveEvaluator.reward."""
    return ProblemSpec("ddave", list(DDAVE_TILES), list(DDAVE_STAT_KEYS), {}, {}, dict(DDAVE_WEIGHTS), dict(DDAVE_WEIGHTS))


def ddave_config(map_shape=(7, 11), solver_power=5000, weights=None, max_diamonds=3, min_spikes=10, target_jumps=2,
                 target_solution=20) -> "_lib.PcgrlDdaveConfig":
    """The C config of include/pcgrl_amd_ddave.h; `weights` replaces entries of the stock table as adjust_param's `rewards`
    does (ddave_prob.py:83-87)."""
    w = dict(DDAVE_WEIGHTS)
    unknown = set(weights or {}) - set(w)
    if unknown:
        raise ValueError(f"unknown ddave statistics in weights: {sorted(unknown)}")
    w.update(weights or {})
    cfg = _lib.PcgrlDdaveConfig()
    cfg.h, cfg.w, cfg.solver_power = int(map_shape[0]), int(map_shape[1]), int(solver_power)
    cfg.max_diamonds, cfg.min_spikes = int(max_diamonds), int(min_spikes)
    cfg.target_jumps, cfg.target_solution = int(target_jumps), int(target_solution)
    for i, k in enumerate(DDAVE_REWARD_ORDER):
        cfg.weight[i] = float(w[k])
    return cfg


class DDaveEvaluator(PlaythroughEvaluator):
    """Evaluates batches of Dangerous Dave maps (1..16 rows x 1..32 columns) on one device.  Owns the search workspace: per
    level 20 * (4 * solver_power + 1) bytes of nodes and open list and 12 bytes for each of the C >= 2 * solver_power slots of
    the visited set -- 596 640 bytes at the stock power of 5 000 (C = 16 384), 2.4 GB for max_levels = 4 096.
    Batches above max_levels run as successive launches on the current stream.  No host sync and no CPU fallback.

    evaluate()'s stats are in DDAVE_STAT_KEYS order and its play columns are DDAVE_PLAY_KEYS: the status (5: more than 64
    diamonds), the four stages' iterations, the returned node's x, y, airTime, health and col_key, the diamonds in the level
    and the returned node's depth; moves are indices into DDAVE_MOVES.  A tile id above 6 reads as solid and sets the error.
    reward() is DDaveProblem.get_reward (ddave_prob.py:181-205), measures() counts T = 7 tiles."""

    NAME, TILES, STAT_KEYS, REWARD_ORDER = "ddave", DDAVE_TILES, DDAVE_STAT_KEYS, DDAVE_REWARD_ORDER
    MEASURE_NAMES, BC_NAMES = DDAVE_MEASURE_NAMES, DDAVE_BC_NAMES

    def __init__(self, map_shape=(7, 11), device="cuda:0", solver_power=5000, weights=None, max_diamonds=3, min_spikes=10,
                 target_jumps=2, target_solution=20, max_levels=4096):
        self.max_diamonds, self.min_spikes = int(max_diamonds), int(min_spikes)
        self.target_jumps, self.target_solution = int(target_jumps), int(target_solution)
        super().__init__(map_shape, device, solver_power, max_levels, ddave_spec,
                         lambda shape, power: ddave_config(shape, power, weights, max_diamonds, min_spikes, target_jumps,
                                                           target_solution))

    def _bounds(self):
        """get_reward's ranges (ddave_prob.py:184-193)"""
        inf = math.inf
        return {"player": (1, 1), "exit": (1, 1), "diamonds": (-inf, self.max_diamonds), "dist-floor": (0, 0), "key": (1, 1),
                "spikes": (self.min_spikes, inf), "regions": (1, 1), "num-jumps": (inf, inf), "dist-win": (-inf, -inf),
                "sol-length": (inf, inf)}

    def episode_over(self, stats):
        """DDaveProblem.get_episode_over (ddave_prob.py:218-220): bool [n]"""
        s = self._stats_arg(stats)
        return (s[:, 10] >= self.target_solution) & (s[:, 7] > self.target_jumps)
