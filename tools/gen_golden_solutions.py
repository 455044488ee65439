"""Sokoban solutions, recorded from the REFERENCE's own solver on the CPU (through oracle/ref_env.py)
-> tests/golden/solutions/*.npz.  Data only; needs the reference tree; about a minute on eight cores.

    python tools/gen_golden_solutions.py

The answer recorded for a map is what SokobanProblem.get_stats(map) returns: stats["solution"] (sokoban_prob.py:178), a list of
the reference's `directions` dicts, stored as indices into that list (engine.py:3), and stats["dist-win"].

(a) fixture_solutions.npz: every level of the committed solver fixtures (tests/golden/stats_sokoban*.npz) whose stored
    sol-length is > 0, with its solution.  Levels with sol-length 0 are NOT re-run (one dense unsolved level takes the
    reference ten minutes): their answer follows from the stored statistics -- length 0 where the statistics show the solver's
    precondition, -1 where they do not.  Layout: `source` ("<file>:<key>" per solved level), `index` (the level's row in that
    array), `offsets` int32 [n + 1] into `moves` int8, `stage` as in (b).
(b) rooms_<H>x<W>.npz: new small-room levels (tests/sokoban_rules.py small_room: the first family of the solver fixtures), forty
    per shape (about one in five is solved), one shape per lanes x mask-width form of the engine and then some; on the shapes wider than 32 most rooms
    straddle column 32 or lie beyond it.  Layout: `grids` uint8 [n, H, W]; `length` int32 [n] (-1: no precondition, 0: the
    solver ran and no stage won); `dist_win` int32 [n]; `stage` int8 [n] (which stage won: 0 BFS, 1..3 A* with balance 1, 0.5,
    0, found by calling the reference's BFSAgent / AStarAgent in _run_game's order; -1: none); `tie` bool [n]: the level's
    solution changes when `directions` is taken in reverse order (tests/sokoban_rules.py solve); `offsets`, `moves` as above;
    `solver_power`.

The script fails unless the plain-Python rules of tests/sokoban_rules.py reproduce every recorded answer, every solution replays
to a win, every shape has at least three solved levels, BFS-won and A*-won levels both exist (counted over (a) and (b)) and some
level tells the order of `directions` apart.  It prints the per-stage counts.
"""
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import sokoban_rules as sr  # noqa: E402
import ref_env  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "solutions")
POWER = 10000  # the reference's default solver_power (what the stored statistics were answered with)
TILES = ["empty", "solid", "player", "crate", "target"]
# (file, key suffix) of every fixture array answered with the default solver_power, and the huge levels (own powers, none solved)
FIXTURES = [("stats_sokoban.npz", ""), ("stats_sokoban_solver.npz", ""),
            ("stats_sokoban_solver_shapes.npz", "_8x8"), ("stats_sokoban_solver_shapes.npz", "_20x20"),
            ("stats_sokoban_solver_shapes.npz", "_30x30"), ("stats_sokoban_solver_wide.npz", "_20x40"),
            ("stats_sokoban_solver_wide.npz", "_48x33"), ("stats_sokoban_solver_wide.npz", "_62x62")]
EXPECT_SOLVED = {"stats_sokoban.npz:": 5, "stats_sokoban_solver.npz:": 21, "stats_sokoban_solver_shapes.npz:_8x8": 1,
                 "stats_sokoban_solver_shapes.npz:_20x20": 3, "stats_sokoban_solver_shapes.npz:_30x30": 0,
                 "stats_sokoban_solver_wide.npz:_20x40": 1, "stats_sokoban_solver_wide.npz:_48x33": 3,
                 "stats_sokoban_solver_wide.npz:_62x62": 1}
# one shape per (lanes per map, mask width) form: 8/32, 16/32, 32/32 (twice), 64/32, 32/64, 64/64 (twice)
ROOM_SHAPES = [(8, 8), (16, 16), (20, 20), (30, 30), (40, 24), (20, 40), (48, 33), (62, 62)]
N_ROOMS = 40  # (about one level in five of this family is solved)

_DIR_INDEX = {(-1, 0): 0, (1, 0): 1, (0, -1): 2, (0, 1): 3}


def _codes(solution):
    return [_DIR_INDEX[(d["x"], d["y"])] for d in solution]


def _reference_state(grid):
    """the State _run_game builds for a map (sokoban_prob.py:100-126)"""
    from control_pcgrl.envs.probs.sokoban.sokoban.engine import State
    chars = " #@$."
    w = grid.shape[1]
    lines = ["#" * (w + 2)] + ["#" + "".join(chars[int(t)] for t in row) + "#" for row in grid] + ["#" * (w + 2), ""]
    state = State()
    state.stringInitialize(lines)
    return state


_CORES = {}


def _core(shape):
    """the reference env of a map shape (rl/envs.py make_env), one per process"""
    if shape not in _CORES:
        _CORES[shape] = ref_env.make_reference_env(ref_env.make_cfg("sokoban", "narrow", shape), seed=0).unwrapped
    return _CORES[shape]


def reference_answer(job):
    """-> (moves or None, dist-win, stage) of one map, from the reference"""
    grid, power, want_stage = job
    from control_pcgrl.envs.probs.sokoban.sokoban.engine import AStarAgent, BFSAgent
    core = _core(tuple(grid.shape))
    prob = core._prob
    prob._solver_power = int(power)
    stats = prob.get_stats(core.get_string_map(grid, prob.get_tile_types()))
    if "solution" not in stats:
        return None, int(stats["dist-win"]), -1
    moves, stage = _codes(stats["solution"]), -1
    if moves and want_stage:  # _run_game's order, until the stage that wins
        state = _reference_state(grid)
        for stage, balance in enumerate((None, 1, 0.5, 0)):
            if balance is None:
                sol, node, _ = BFSAgent().getSolution(state, int(power))
            else:
                sol, node, _ = AStarAgent().getSolution(state, balance, int(power))
            if node.checkWin():
                assert _codes(sol) == moves, "the stage that wins returns the recorded solution"
                break
        else:
            raise AssertionError("no stage wins a solved level")
    return moves, int(stats["dist-win"]), stage


def check_against_rules(grid, power, moves, dist_win, stage=None):
    """the rules as the tests state them: agreement is checked here already"""
    if moves is None:
        assert not sr.precondition(grid)
        return
    assert sr.precondition(grid)
    mine, dw, st = sr.solve(grid, power)
    assert mine == moves and dw == dist_win and (stage is None or st == stage), (grid, moves, mine, dist_win, dw, stage, st)
    if moves:
        assert sr.replay(grid, moves) == (True, True), (grid, moves)


def fixture_solutions(pool):
    jobs, where = [], []
    for fname, suffix in FIXTURES:
        z = np.load(os.path.join(GOLDEN, fname))
        grids, stats = z["grids" + suffix], z["stats" + suffix]
        solved = np.flatnonzero(stats[:, 5] > 0)
        assert len(solved) == EXPECT_SOLVED[f"{fname}:{suffix}"], (fname, suffix, len(solved))
        for i in solved:
            jobs.append((grids[i], POWER, True))
            where.append((f"{fname}:grids{suffix}", int(i), int(stats[i, 5])))
    huge = np.load(os.path.join(GOLDEN, "stats_sokoban_solver_huge.npz"))
    assert not (huge["stats"][:, 5] > 0).any(), "a solved level of more than 128 pairs: record it"
    assert len(jobs) == 35
    answers = pool.map(reference_answer, jobs, chunksize=1)
    sols = []
    stages = np.array([a[2] for a in answers], np.int8)
    for (grid, _, _), (src, i, sol_len), (moves, dw, _) in zip(jobs, where, answers):
        assert moves is not None and len(moves) == sol_len and dw == 0, (src, i)
        assert sr.replay(grid, moves) == (True, True), (src, i)
        if grid.shape[0] * grid.shape[1] <= 400:  # (the plain-Python rules: small maps only, the rest is the replay's)
            check_against_rules(grid, POWER, moves, dw)
        sols.append(moves)
    path = os.path.join(OUT, "fixture_solutions.npz")
    np.savez_compressed(path, source=np.array([w[0] for w in where]), index=np.array([w[1] for w in where], np.int32),
                        offsets=np.cumsum([0] + [len(s) for s in sols]).astype(np.int32),
                        moves=np.concatenate([np.array(s, np.int8) for s in sols]), stage=stages,
                        solver_power=np.int32(POWER))
    counts = np.array([int((stages == s).sum()) for s in range(4)])
    print(f"{os.path.relpath(path, ROOT)}: {len(sols)} solutions, lengths {min(map(len, sols))}..{max(map(len, sols))}, won by "
          f"stage {counts.tolist()}, {os.path.getsize(path)} bytes", flush=True)
    return path, counts


def room_levels(pool, stage_counts):
    paths, n_tie = [], 0
    for k, shape in enumerate(ROOM_SHAPES):
        rng = np.random.default_rng(4100 + k)
        grids = []
        for _ in range(N_ROOMS):
            wide = shape[1] > 32 and rng.random() < 0.7  # rooms that straddle column 32 or lie beyond it
            grids.append(sr.small_room(rng, shape, x_from=26 if wide else None))
        grids = np.array(grids, np.uint8)
        answers = pool.map(reference_answer, [(g, POWER, True) for g in grids], chunksize=1)
        length, dist_win, stage, tie, sols = [], [], [], [], []
        for g, (moves, dw, st) in zip(grids, answers):
            check_against_rules(g, POWER, moves, dw, st)
            length.append(-1 if moves is None else len(moves))
            dist_win.append(dw)
            stage.append(st)
            tie.append(bool(moves) and sr.solve(g, POWER, directions=sr.DIRECTIONS[::-1])[0] != moves)
            sols.append(moves or [])
        length, stage, tie = np.array(length, np.int32), np.array(stage, np.int8), np.array(tie)
        solved = int((length > 0).sum())
        assert solved >= 3, f"{shape}: only {solved} solved levels"
        if shape[1] > 32:
            cols = [np.flatnonzero((g != sr.SOLID).any(0)) for g in grids]
            assert sum(c.min() < 32 <= c.max() for c in cols) >= 3, f"{shape}: no rooms across column 32"
        for s in range(4):
            stage_counts[s] += int((stage == s).sum())
        n_tie += int(tie.sum())
        path = os.path.join(OUT, f"rooms_{shape[0]}x{shape[1]}.npz")
        np.savez_compressed(path, grids=grids, length=length, dist_win=np.array(dist_win, np.int32), stage=stage, tie=tie,
                            offsets=np.cumsum([0] + [len(s) for s in sols]).astype(np.int32),
                            moves=np.concatenate([np.array(s, np.int8) for s in sols]), solver_power=np.int32(POWER))
        print(f"{os.path.relpath(path, ROOT)}: {len(grids)} levels, {solved} solved (longest {length.max()}), "
              f"{int((length == 0).sum())} unsolved, {int((length < 0).sum())} without the precondition, won by stage "
              f"{[int((stage == s).sum()) for s in range(4)]}, {int(tie.sum())} tell the order of directions apart, "
              f"{os.path.getsize(path)} bytes", flush=True)
        paths.append(path)
    print("won by BFS / A* balance 1 / 0.5 / 0:", stage_counts.tolist(), "; solutions that change with reversed directions:", n_tie)
    assert stage_counts[0] > 0 and stage_counts[1:].sum() > 0, "BFS-won and A*-won levels must both exist"
    assert n_tie > 0, "the fixtures do not tell the order of directions apart"
    return paths


def main():
    assert ref_env.available(), "reference tree not present"
    os.makedirs(OUT, exist_ok=True)
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        first, counts = fixture_solutions(pool)
        paths = [first] + room_levels(pool, counts)
    for p in paths:
        assert os.path.getsize(p) <= 64 * 1024, p


if __name__ == "__main__":
    main()
