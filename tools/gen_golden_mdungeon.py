"""MiniDungeon levels, recorded from the REFERENCE on the CPU (through oracle/ref_env.py's shim) ->
tests/golden/mdungeon/*.npz.  Data only; needs the reference tree; a few minutes on one core.  Not for the GPU machine.

    python tools/gen_golden_mdungeon.py

The reference can no longer construct MDungeonProblem (it calls Problem.__init__() without cfg), so what is recorded is what is
still callable: get_stats, get_reward and get_episode_over on an instance made without __init__ and given its plain
attributes.  The searches are observed through subclasses of AStarAgent and BFSAgent whose getSolution calls the reference's
and keeps what it returned.

md_<H>x<W>_p<power>.npz (maps of tests/mdungeon_levels.py and hand-built ones; `names` says what made each):
  grids        uint8 [n][H][W]; power int32
  stats        int32 [n][11]: get_stats(map) in its dict order (`stat_keys`)
  stage_iters  int32 [n][4], stage_won int8 [n][4]: per getSolution call its iteration count and whether its state had won
               (-1: the stage did not run); stage_node int32 [n][4][3]: the returned node's x, y and depth (-1: not run) --
               a stage that does not win returns its best node, which only the last stage passes on
  moves        int8 [n][cap], length int32 [n]: the returned action list as indices into engine.directions, -1 past the end
  play         int32 [n][12]: the device's play record (include/pcgrl_amd_mdungeon.h) built from the reference's values:
               status, the four iteration counts, the returned state's player x, y, health, potions, treasures, enemies,
               len(sol)
  rew_new, rew_old int32 [m][11]; rew_bits uint64 [m] (get_reward as a float64 pattern), over bool [m] (get_episode_over of
               rew_new), with the stock parameters; rew_bits_custom / over_custom with custom_weights float64 [9] (the
               reward's order of summation), custom_params int32 [4] (max_enemies, max_potions, max_treasures,
               target_solution) and custom_target_col_enemies float64
meas_<H>x<W>.npz: the measures and the diversity, recorded as tools/gen_golden_ddave.py does (the reference's text compiled
  through `ast`; tools/gen_golden_measures.py's docstring has the layout), with T = 8.

The script refuses to write unless tests/mdungeon_rules.py reproduces every recorded field, its tuple key and the string of
State.getKey agree one to one on every node of every recorded level, the sets hold each of CASES, and each wrong rule of
mdungeon_rules.WRONG_RULES fails at least one fixture.  Files are written with fixed zip timestamps, so a rerun is
byte-identical.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_golden_measures as gm  # noqa: E402
import mdungeon_levels as ml  # noqa: E402
import mdungeon_rules as R  # noqa: E402
import ref_env  # noqa: E402
from gen_golden_microstructure import write_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mdungeon")
STOCK = (11, 7, 5000)
SMALL_SHAPES = [(1, 1), (1, 2), (1, 3), (2, 3), (3, 4), (5, 13), (16, 32)]
SMALL_POWERS = [1, 2, 50, 500]
MEAS_SHAPES = [(1, 1), (1, 32), (16, 1), (5, 2), (5, 13), (11, 7), (16, 32)]
CUSTOM_WEIGHTS = {"player": 1.5, "exit": 2.0, "potions": 0.3, "treasures": 0.7, "enemies": 1.1, "regions": 4.0,
                  "col-enemies": 0.9, "dist-win": 0.05, "sol-length": 0.6}
CUSTOM_PARAMS = (3, 1, 2, 5)  # max_enemies, max_potions, max_treasures, target_solution
CUSTOM_TARGET_COL_ENEMIES = 0.25
CASES = ["won at stage 1", "won at stage 2", "won at stage 3", "won at stage 4", "no win, budget hit", "no win, open list emptied",
         "0 players", "2 players", "0 exits", "2 exits", "2 regions", "a popped lost node", "a potion taken at health 5",
         "a potion clamped from health 4", "an ogre met at health 1", "negative dist-win", "an already-visited pop",
         "a move into a wall", "the same item set at two healths", "power 1"]
MAX_FILE_BYTES = 100 * 1024


def make_problem(MDungeonProblem, h, w, power, weights=None, params=(6, 2, 3, 20), target_col_enemies=0.5):
    prob = MDungeonProblem.__new__(MDungeonProblem)  # __init__ raises TypeError in this checkout
    prob._width, prob._height, prob._solver_power = w, h, power
    prob._max_enemies, prob._max_potions, prob._max_treasures, prob._target_solution = params
    prob._target_col_enemies = target_col_enemies
    prob._reward_weights = dict(R.WEIGHTS)
    prob._reward_weights.update(weights or {})
    return prob


class Recorder:
    def __init__(self):
        from control_pcgrl.envs.probs.mdungeon import mdungeon_prob
        from control_pcgrl.envs.probs.mdungeon.mdungeon import engine
        self.MDungeonProblem, self.engine = mdungeon_prob.MDungeonProblem, engine
        self.calls = calls = []

        class AStar(engine.AStarAgent):
            def getSolution(self, state, balance=1, maxIterations=-1):
                ret = super().getSolution(state, balance, maxIterations)
                calls.append(ret)
                return ret

        class BFS(engine.BFSAgent):
            def getSolution(self, state, maxIterations=-1):
                ret = super().getSolution(state, maxIterations)
                calls.append(ret)
                return ret

        mdungeon_prob.AStarAgent, mdungeon_prob.BFSAgent = AStar, BFS
        assert [(d["x"], d["y"]) for d in engine.directions] == list(R.DIRECTIONS)
        self.seconds = 0.0

    def level(self, prob, m):
        """(stats, stage_iters, stage_won, actions, play, stage_node) of one map, all from the reference"""
        assert prob.get_tile_types() == R.TILES
        del self.calls[:]
        t0 = time.perf_counter()
        stats = prob.get_stats([[R.TILES[t] for t in row] for row in m])
        self.seconds += time.perf_counter() - t0
        assert list(stats) == R.STAT_KEYS
        iters, won, nodes = [0] * 4, [-1] * 4, [[-1] * 3 for _ in range(4)]
        acts, play = [], [-1] + [0] * 11
        for s, (sol, node, it) in enumerate(self.calls):
            iters[s], won[s] = it, int(node.checkWin())
            nodes[s] = [node.state.player["x"], node.state.player["y"], node.depth]
            assert len(sol) == node.depth
        if self.calls:
            sol, node, _ = self.calls[-1]
            acts = [self.engine.directions.index(d) for d in sol]
            pl = node.state.player
            status = len(self.calls) if won[len(self.calls) - 1] else 0
            play = [status] + iters + [pl["x"], pl["y"], pl["health"], pl["potions"], pl["treasures"], pl["enemies"], len(sol)]
            game = node.getGameStatus()
            assert game["col_potions"] == stats["col-potions"] and game["col_treasures"] == stats["col-treasures"]
            assert game["col_enemies"] == stats["col-enemies"]
        return [int(stats[k]) for k in R.STAT_KEYS], iters, won, acts, play, nodes


def hand_levels(h, w):
    """the failing preconditions and the health quirks, where the shape has room"""
    out = []
    if h * w >= 4:
        base = np.zeros((h, w), np.uint8)
        flat = base.ravel()
        flat[0], flat[2] = R.PLAYER, R.EXIT
        out.append(("one-each", base.copy()))
        for name, at, tile in (("no-player", 0, R.EMPTY), ("two-players", 3, R.PLAYER), ("no-exit", 2, R.EMPTY),
                               ("two-exits", 3, R.EXIT)):
            m = base.copy()
            m.ravel()[at] = tile
            out.append((name, m))
    if w >= 5:
        m = np.zeros((h, w), np.uint8)
        m[0, 0], m[0, 2] = R.PLAYER, R.EXIT
        m[:, 3] = R.SOLID
        out.append(("two-regions", m))
    if w >= 5:
        # one corridor: the player, three ogres, the door -- the third ogre is met at health 1 and every route ends lost
        m = np.full((h, w), R.SOLID, np.uint8)
        m[h // 2, :5] = (R.PLAYER, R.OGRE, R.OGRE, R.OGRE, R.EXIT)
        m[h // 2, 5:] = R.EMPTY
        out.append(("three-ogres", m))
        # a potion right of the player at full health, then the door
        m = np.full((h, w), R.SOLID, np.uint8)
        m[h // 2, :5] = (R.EMPTY, R.PLAYER, R.POTION, R.EMPTY, R.EXIT)
        out.append(("potion-at-full-health", m))
        # goblin, potion (4 -> 5, clamped), door
        m = np.full((h, w), R.SOLID, np.uint8)
        m[h // 2, :5] = (R.PLAYER, R.GOBLIN, R.POTION, R.EMPTY, R.EXIT)
        out.append(("goblin-then-potion", m))
    if h >= 2 and w >= 5:
        # two routes to the door over the same items in either order: potion then goblin (health 4), goblin then potion (5)
        m = np.zeros((h, w), np.uint8)
        m[0, :5] = (R.PLAYER, R.POTION, R.GOBLIN, R.EMPTY, R.EXIT)
        m[1, :5] = (R.EMPTY, R.EMPTY, R.EMPTY, R.EMPTY, R.EMPTY)
        out.append(("two-orders", m))
    if w >= 10:
        # a one-cell-high corridor: the door two steps left of the player, a trail of treasures leading away.  Every A* is
        # drawn down the trail (a treasure is worth 4 steps); the BFS finds the moves to the left at once.
        m = np.full((h, w), R.SOLID, np.uint8)
        m[h // 2] = R.TREASURE
        m[h // 2, :3] = (R.EXIT, R.EMPTY, R.PLAYER)
        out.append(("treasure-lure", m))
    return out


def cases_of(m, power, stats, won, play, trace):
    got = set()
    for s in range(4):
        if won[s] == 1:
            got.add(f"won at stage {s + 1}")
    if play[0] == 0:
        got.add("no win, budget hit" if play[4] == power else "no win, open list emptied")
    others_fine = lambda skip: all(stats[j] == 1 for j in (0, 1, 5) if j != skip)  # noqa: E731
    if stats[0] == 0:
        got.add("0 players")
    if stats[0] == 2 and others_fine(0):
        got.add("2 players")
    if stats[1] == 0 and others_fine(1):
        got.add("0 exits")
    if stats[1] == 2 and others_fine(1):
        got.add("2 exits")
    if stats[5] == 2 and others_fine(5):
        got.add("2 regions")
    for flag, case in (("lost-pop", "a popped lost node"), ("potion-at-5", "a potion taken at health 5"),
                       ("potion-from-4", "a potion clamped from health 4"), ("ogre-at-1", "an ogre met at health 1"),
                       ("visited-pop", "an already-visited pop"), ("wall", "a move into a wall"),
                       ("same-items-two-healths", "the same item set at two healths")):
        if flag in trace:
            got.add(case)
    if stats[9] < 0:
        got.add("negative dist-win")
    if power == 1 and play[0] >= 0:
        got.add("power 1")
    return got


def candidates(h, w, power, seed):
    """(name, map): the hand-built levels, then generated ones -- for the stock set about 200; for the small sets a pool of
    which the levels that show a stage-2, -3 or -4 win are kept first, then the others up to 40"""
    rng = np.random.default_rng(seed)
    named = hand_levels(h, w)
    if (h, w, power) == STOCK:
        quick = [g for g in ml.GENERATORS if g is not ml.guarded_exit]
        for i in range(186):
            gen = quick[i % len(quick)]
            named.append((f"{gen.__name__}-{i}", gen(rng, h, w)))
        for i in range(4):  # four searches of 5 000 iterations each: a few are enough, the rules replay them in every test run
            named.append((f"guarded_exit-{i}", ml.guarded_exit(rng, h, w)))
        return named
    pool = [(f"{ml.GENERATORS[i % len(ml.GENERATORS)].__name__}-{i}", ml.GENERATORS[i % len(ml.GENERATORS)](rng, h, w))
            for i in range(240 if h * w <= 64 else 120)]
    rare = [(k, m) for k, m in pool if R.outputs(m, power)[3][0] in (2, 3, 4)]
    rest = [(k, m) for k, m in pool if not any(k == r[0] for r in rare)]
    return named + rare[:12] + rest[:40 - min(12, len(rare))]


def reward_pairs(rng, stats):
    """pairs of recorded statistics, and perturbed ones that cross the reward's ranges in both directions"""
    n = len(stats)
    new, old = [], []
    for _ in range(48):
        i, j = rng.integers(0, n, 2)
        new.append(list(stats[i]))
        old.append(list(stats[j]))
    for _ in range(48):
        a, b = list(stats[rng.integers(0, n)]), list(stats[rng.integers(0, n)])
        for s in (a, b):
            for j in rng.choice(11, 3, replace=False):
                s[j] = int(rng.integers(0, 25)) - (12 if j == 9 else 0)
        new.append(a)
        old.append(b)
    return np.asarray(new, np.int32), np.asarray(old, np.int32)


def bits(values):
    return np.asarray([float(v) for v in values], np.float64).view(np.uint64)


def record_set(rec, h, w, power, seed, seen, wrong_fails):
    named = candidates(h, w, power, seed)
    prob = make_problem(rec.MDungeonProblem, h, w, power)
    rows = [rec.level(prob, m) for _, m in named]
    cap = max(1, max(len(r[3]) for r in rows))
    n = len(named)
    stats, iters, won = np.zeros((n, 11), np.int32), np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int8)
    moves, length, play = np.full((n, cap), -1, np.int8), np.zeros(n, np.int32), np.zeros((n, 12), np.int32)
    stage_node = np.full((n, 4, 3), -1, np.int32)
    for i, (name, m) in enumerate(named):
        st, it, wn, acts, pl, sn = rows[i]
        mv, ln = (acts + [-1] * cap)[:cap], len(acts)
        trace, stages = set(), []
        mine = R.outputs(m, power, cap, key_check={}, trace=trace, stages=stages)  # (the two keys are compared inside)
        assert mine == (st, mv, ln, pl), ((h, w, power), name, mine, (st, mv, ln, pl))
        assert stages == [x for x in sn if x[2] >= 0], ((h, w, power), name, stages, sn)
        stage_node[i] = sn
        assert [x if x >= 0 else 0 for x in it] == pl[1:5] or pl[0] < 0
        stats[i], iters[i], won[i], moves[i], length[i], play[i] = st, it, wn, mv, ln, pl
        for c in cases_of(m, power, st, wn, pl, trace):
            seen.setdefault(c, []).append(f"{h}x{w}p{power}:{name}")
        if pl[0] >= 0:
            for rule in R.WRONG_RULES:
                wrong_stages = []
                wrong_fails[rule] += R.outputs(m, power, cap, wrong=rule, stages=wrong_stages) != mine or wrong_stages != stages
    rng = np.random.default_rng(seed + 77)
    new, old = reward_pairs(rng, stats)
    custom = make_problem(rec.MDungeonProblem, h, w, power, CUSTOM_WEIGHTS, CUSTOM_PARAMS, CUSTOM_TARGET_COL_ENEMIES)
    rew, over, rew_c, over_c = [], [], [], []
    for a, b in zip(new, old):
        da, db = ({k: int(v) for k, v in zip(R.STAT_KEYS, s)} for s in (a, b))
        rew.append(prob.get_reward(da, db))
        over.append(bool(prob.get_episode_over(da, db)))
        rew_c.append(custom.get_reward(da, db))
        over_c.append(bool(custom.get_episode_over(da, db)))
        assert bits([R.reward(a, b)]) == bits([rew[-1]]) and R.episode_over(a) == over[-1]
        assert bits([R.reward(a, b, CUSTOM_WEIGHTS, *CUSTOM_PARAMS[:3])]) == bits([rew_c[-1]])
        assert R.episode_over(a, CUSTOM_TARGET_COL_ENEMIES, CUSTOM_PARAMS[3]) == over_c[-1]
    return {
        "grids": np.stack([m for _, m in named]).astype(np.uint8), "power": np.int32(power), "stats": stats,
        "stage_iters": iters, "stage_won": won, "stage_node": stage_node, "moves": moves, "length": length, "play": play,
        "rew_new": new, "rew_old": old, "rew_bits": bits(rew), "over": np.asarray(over), "rew_bits_custom": bits(rew_c),
        "over_custom": np.asarray(over_c), "custom_weights": np.asarray([CUSTOM_WEIGHTS[k] for k in R.REWARD_ORDER], np.float64),
        "custom_params": np.asarray(CUSTOM_PARAMS, np.int32),
        "custom_target_col_enemies": np.float64(CUSTOM_TARGET_COL_ENEMIES), "names": np.asarray([k for k, _ in named]),
        "stat_keys": np.asarray(R.STAT_KEYS),
    }


def main():
    assert ref_env.available(), "the reference tree is needed"
    rec = Recorder()
    seen, files = {}, {}
    wrong_fails = dict.fromkeys(R.WRONG_RULES, 0)
    sets = [STOCK] + [(h, w, p) for h, w in SMALL_SHAPES for p in SMALL_POWERS]
    for seed, (h, w, power) in enumerate(sets):
        z = record_set(rec, h, w, power, 800 + seed, seen, wrong_fails)
        files[f"md_{h}x{w}_p{power}"] = z
        pl = z["play"]
        print(f"{h}x{w} power {power}: {len(pl)} levels, {(pl[:, 0] >= 0).sum()} searched, {(pl[:, 0] > 0).sum()} won, "
              f"up to {pl[:, 1:5].sum(1).max()} iterations, dist-win down to {z['stats'][:, 9].min()}", flush=True)
    missing = [c for c in CASES if not seen.get(c)]
    assert not missing, f"no level shows: {missing}"
    print("fixtures failed by each wrong rule:", wrong_fails)
    blind = [k for k, v in wrong_fails.items() if v == 0]
    assert not blind, f"the fixture set does not tell these rules apart: {blind}"
    # the measures and the diversity: the reference's own functions, T = 8
    gm.mn.N_TILES.setdefault("mdungeon", len(R.TILES))
    ref = gm.reference_functions()
    meas = {}
    for si, shape in enumerate(MEAS_SHAPES):
        z = gm.generate("mdungeon", shape, ref, seed=9700 + si)
        assert z["grids"].max() < len(R.TILES) and z["counts"].shape[1] == len(R.TILES)
        meas[("mdungeon", shape)] = z
        files[f"meas_{shape[0]}x{shape[1]}"] = z
    gm.check_worth(meas)
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, arrays in files.items():
        path = os.path.join(OUT, name + ".npz")
        write_npz(path, arrays)
        size = os.path.getsize(path)
        assert size <= MAX_FILE_BYTES, (path, size)
        total += size
    for c in CASES:
        print(f"{c}: {len(seen[c])} levels, e.g. {seen[c][0]}")
    print(f"reference get_stats on all recorded levels: {rec.seconds:.1f} s")
    print(total, "bytes in all")


if __name__ == "__main__":
    main()
