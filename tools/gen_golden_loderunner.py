"""Lode Runner levels, recorded from the REFERENCE on the CPU (through oracle/ref_env.py's shim) ->
tests/golden/loderunner/*.npz.  Data only; needs the reference tree; about a minute on one core.  Not for the GPU machine.

    python tools/gen_golden_loderunner.py

The reference can no longer construct LoderunnerProblem (it calls Problem.__init__() without cfg), so what is recorded is what
is still callable: the body of LoderunnerProblem.get_stats on an instance made without __init__, which calls
loderunner/engine.py:get_score.  The engine abandons an evaluation after one second of wall clock (engine.py:254, 287, 293);
here `engine.time` is replaced, in this process only, by a clock that stands still, so a fixture is the engine's answer with
the limit never biting.  For the 8 x 12 sets the untouched engine runs as well: the results must be identical, and the longest
elapsed time is printed -- the limit does not bite at the stock size.

Per set (one file: a map shape, levels of tests/loderunner_levels.py) and per level:
  grids        uint8 [n][H][W]
  stats        float64 [n][5]: get_stats(map) in its dict order (`stat_keys`)
  landing      int32 [n][2]: get_starting_point's cell; (-1, -1) where player != 1 and nothing was searched
  collected    int32 [n]: the golds collected, those on the fall included
  gold_state   int8 [n][G], gold_dist int16 [n][G]: per gold in row-major order 0 not collected, 1 by its own pair of
               searches, 2 on another gold's path, 3 on the fall, -1 past the last gold; what the gold added to path-length.
               From wrappers around AStar.run, find_all_golds and Node.get_path.
  kind         which generator made the level

The script refuses to write unless tests/loderunner_rules.py reproduces every recorded field and the sets hold each of CASES.
Files are written with fixed zip timestamps, so a rerun is byte-identical.
"""
import io
import os
import sys
import time
import zipfile
from collections import deque

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import loderunner_levels as ll  # noqa: E402
import loderunner_rules as R  # noqa: E402
import ref_env  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "loderunner")
# name: (H, W, [(kind, seed, n), ...])
SETS = {
    "stock_random": (8, 12, [("random", 1, 40), ("chance", 2, 24)]),
    "stock_gold": (8, 12, [("gold", 3, 24)]),
    "stock_structured": (8, 12, [("structured", 4, 40)]),
    "stock_detour": (8, 12, [("detour", 26, 6)]),
    "h1w1": (1, 1, [("random", 5, 4), ("chance", 6, 12), ("gold", 7, 2)]),
    "h2w1": (2, 1, [("random", 8, 6), ("chance", 9, 16), ("gold", 10, 4)]),
    "h1w5": (1, 5, [("random", 11, 12), ("chance", 12, 8), ("gold", 13, 12)]),
    "h4w4": (4, 4, [("random", 14, 16), ("gold", 15, 16), ("structured", 16, 16)]),
    "h5w7": (5, 7, [("random", 17, 16), ("gold", 18, 16), ("structured", 19, 16)]),
    "h3w9": (3, 9, [("random", 20, 12), ("gold", 21, 12), ("structured", 22, 12)]),
    "h16w32": (16, 32, [("random", 23, 4), ("gold", 24, 2), ("structured", 25, 6)]),
}
CASES = ["win -1", "win 1", "win strictly between", "win 1/(1+G)", "0 players", "2 players", "fall of at least 2 rows",
         "gold collected during the fall", "gold on the landing cell", "fall stopped by a rope", "player on the bottom row",
         "search enters the left-behind player", "state 2 from a to-goal path", "state 2 from a to-start path",
         "gold reached with no way back"] + ["move " + n for n in R.MOVE_NAMES] + ["path longer than the BFS distance"]


class StoppedClock:
    @staticmethod
    def time():
        return 0.0


def make_levels(kind, seed, n, h, w):
    if kind == "chance":  # the player count left to _prob: 0, 1 or more
        rng = np.random.default_rng(seed)
        return np.stack([ll.random_level(rng, h, w, keep_players=True) for _ in range(n)])
    if kind == "detour":  # the first n gold-heavy levels of the stream with a counted path longer than the BFS distance
        rng, out = np.random.default_rng(seed), []
        while len(out) < n:
            m = ll.gold_level(rng, h, w)
            if has_detour(m):
                out.append(m)
        return np.stack(out)
    return ll.batch(kind, seed, n, h, w)


def has_detour(m):
    record = []
    played = R.clean(m)
    r, c, _ = R.start(played)
    played[r, c] = R.EMPTY
    R.play(m, record=record)
    return any(len(p[0]) - 1 > bfs_steps(played, p[0][-1], p[0][0]) for _, a, b in record if b is not None for p in (a, b))


class Recorder:
    def __init__(self):
        from control_pcgrl.envs.probs.loderunner import engine
        from control_pcgrl.envs.probs.loderunner_prob import LoderunnerProblem
        self.engine = engine
        self.prob = LoderunnerProblem.__new__(LoderunnerProblem)  # __init__ raises TypeError in this checkout
        self.prob.tiles_to_chars = dict(zip(R.TILES, R.CHARS))
        assert self.prob.get_tile_types() == R.TILES
        self.real_time = engine.time
        self.longest = 0.0

    def level(self, m, also_unpatched):
        engine = self.engine
        str_map = [[R.TILES[t] for t in row] for row in m]
        runs, paths, golds_arg, start = [], [], [], []
        o_run, o_find, o_path, o_start = engine.AStar.run, engine.find_all_golds, engine.Node.get_path, engine.get_starting_point

        def run(astar, timer):
            node = o_run(astar, timer)
            runs.append(((astar.root.row, astar.root.col), (astar.goal_row, astar.goal_col), node))
            return node

        def find(root, golds, map2d):
            golds_arg.append(list(golds))
            return o_find(root, golds, map2d)

        def get_path(node):
            path, other = o_path(node)
            actions, k = [], node
            while k.parent is not None:
                actions.append(k.action)
                k = k.parent
            paths.append(((node.row, node.col), path, other, actions))
            return path, other

        def starting(map2d):
            out = o_start(map2d)
            start.append(out)
            return out

        engine.AStar.run, engine.find_all_golds, engine.Node.get_path, engine.get_starting_point = run, find, get_path, starting
        engine.time = StoppedClock
        try:
            stats = self.prob.get_stats(str_map)
        finally:
            engine.AStar.run, engine.find_all_golds, engine.Node.get_path, engine.get_starting_point = o_run, o_find, o_path, o_start
            engine.time = self.real_time
        assert list(stats) == R.STAT_KEYS
        if also_unpatched:
            t0 = time.perf_counter()
            again = self.prob.get_stats(str_map)
            self.longest = max(self.longest, time.perf_counter() - t0)
            assert again == stats, (again, stats)
        all_golds = [(int(r), int(c)) for r, c in np.argwhere(m == R.GOLD)]
        rec = {"stats": [stats[k] for k in R.STAT_KEYS], "landing": (-1, -1), "collected": 0, "state": [0] * len(all_golds),
               "dist": [0] * len(all_golds), "runs": runs, "paths": paths, "via": {}}
        if stats["player"] != 1:
            assert not start and not runs
            return rec
        row, col, on_start = start[0]
        rec["landing"] = (int(row), int(col))
        state = {g: (R.ON_THE_FALL if g in on_start else 0) for g in all_golds}
        dist = {g: 0 for g in all_golds}
        if all_golds:
            golds = golds_arg[0]
            found, total = [], 0
            assert len(paths) % 2 == 0
            for i, (cell, path, other, _) in enumerate(paths):
                if i % 2 == 0:  # to_goal.get_path(): the gold's own pair of searches succeeded
                    assert cell in golds and cell not in found
                    found.append(cell)
                    state[cell], dist[cell] = R.BY_OWN_SEARCHES, len(path)
                    total += len(path)
                for og in other:
                    if og not in found and og in golds:
                        found.append(og)
                        state[og] = R.ON_ANOTHER_PATH
                        rec["via"][og] = "to-goal" if i % 2 == 0 else "to-start"
            assert total == stats["path-length"]
            rec["collected"] = len(found) + len(on_start)
            assert stats["win"] == 1 / (1 + (len(all_golds) - rec["collected"]))
        rec["state"], rec["dist"] = [state[g] for g in all_golds], [dist[g] for g in all_golds]
        return rec


def bfs_steps(m, src, goal):
    seen, todo = {src: 0}, deque([src])
    while todo:
        cell = todo.popleft()
        if cell == goal:
            return seen[cell]
        for mv in R.moves(m, *cell):
            child = (cell[0] + R.DELTA[mv][0], cell[1] + R.DELTA[mv][1])
            if child not in seen:
                seen[child] = seen[cell] + 1
                todo.append(child)
    return None


def cases_of(m, rec):
    got = set()
    players = int((m == R.PLAYER).sum())
    if players == 0:
        got.add("0 players")
    if players == 2:
        got.add("2 players")
    if players != 1:
        return got
    H, W = m.shape
    golds = int((m == R.GOLD).sum())
    win = rec["stats"][3]
    if win == -1:
        got.add("win -1")
    elif win == 1:
        got.add("win 1")
    else:
        got.add("win strictly between")
        if rec["collected"] == 0:
            got.add("win 1/(1+G)")
    pr, pc = [int(v) for v in np.argwhere(m == R.PLAYER)[0]]
    lr, lc = rec["landing"]
    if lr - pr >= 2:
        got.add("fall of at least 2 rows")
    all_golds = [(int(r), int(c)) for r, c in np.argwhere(m == R.GOLD)]
    for g, s in zip(all_golds, rec["state"]):
        if s == R.ON_THE_FALL:
            got.add("gold on the landing cell" if g == (lr, lc) else "gold collected during the fall")
    if lr > pr and m[lr, lc] == R.ROPE and lr != H - 1 and m[lr + 1, lc] not in R.SUPPORT:
        got.add("fall stopped by a rope")
    if pr == H - 1:
        got.add("player on the bottom row")
    for via in rec["via"].values():
        got.add(f"state 2 from a {via} path")
    by_pair = {}
    for src, goal, node in rec["runs"]:
        by_pair[(src, goal)] = node
    for (src, goal), node in by_pair.items():
        if src == (lr, lc) and node is not None and by_pair.get((goal, src), 0) is None:
            got.add("gold reached with no way back")
    played = R.clean(m)
    played[lr, lc] = R.EMPTY
    for cell, path, _, actions in rec["paths"]:
        for a in actions:
            got.add("move " + a)
        d = bfs_steps(played, path[-1], path[0])
        assert d is not None and d <= len(path) - 1
        if len(path) - 1 > d:
            got.add("path longer than the BFS distance")
    if (lr, lc) != (pr, pc) and golds:
        pushed = set()
        R.play(m, pushed=pushed)
        if (pr, pc) in pushed:
            got.add("search enters the left-behind player")
    return got


def check_rules(m, rec, where):
    """tests/loderunner_rules.py reproduces every recorded field"""
    cap = max(1, len(rec["state"]))
    stats, play, gs, gd = R.outputs(m, cap)
    assert stats == [float(s) for s in rec["stats"]], (where, stats, rec["stats"])
    searched = int(rec["stats"][0] == 1)
    assert play == [searched, rec["landing"][0], rec["landing"][1], rec["collected"]], (where, play, rec["landing"])
    n = len(rec["state"])
    assert gs[:n] == rec["state"] and gd[:n] == rec["dist"], (where, gs, rec["state"], gd, rec["dist"])
    if searched:
        record = []
        R.play(m, record=record)
        ref = {(src, goal): node for src, goal, node in rec["runs"]}
        paths = {(p[1][-1], p[1][0]): p for p in rec["paths"]}
        start = tuple(rec["landing"])
        assert len(record) * 2 >= len(ref) >= len(record)
        for g, to_goal, to_start in record:
            assert (to_goal is None) == (ref[(start, g)] is None), (where, g)
            if to_goal is not None:
                assert (to_start is None) == (ref[(g, start)] is None), (where, g)
            if to_start is not None:
                for (cells, taken), key in ((to_goal, (start, g)), (to_start, (g, start))):
                    assert cells == [tuple(int(v) for v in c) for c in paths[key][1]], (where, key)
                    assert [R.MOVE_NAMES[a] for a in taken] == paths[key][3], (where, key)


def write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    assert ref_env.available(), "the reference tree is needed"
    rec = Recorder()
    seen, files, total = {}, {}, 0
    for name, (h, w, parts) in SETS.items():
        grids, kinds, recs = [], [], []
        for kind, seed, n in parts:
            for i, m in enumerate(make_levels(kind, seed, n, h, w)):
                r = rec.level(m, also_unpatched=(h, w) == (8, 12))
                check_rules(m, r, (name, kind, seed, i))
                for c in cases_of(m, r):
                    seen.setdefault(c, []).append(f"{name}:{kind}{seed}#{i}")
                grids.append(m)
                kinds.append(kind)
                recs.append(r)
        cap = max(1, max(len(r["state"]) for r in recs))
        gs = np.full((len(recs), cap), -1, dtype=np.int8)
        gd = np.zeros((len(recs), cap), dtype=np.int16)
        for i, r in enumerate(recs):
            gs[i, :len(r["state"])] = r["state"]
            gd[i, :len(r["dist"])] = r["dist"]
        files[name] = {
            "grids": np.stack(grids).astype(np.uint8), "stats": np.asarray([r["stats"] for r in recs], dtype=np.float64),
            "landing": np.asarray([r["landing"] for r in recs], dtype=np.int32),
            "collected": np.asarray([r["collected"] for r in recs], dtype=np.int32), "gold_state": gs, "gold_dist": gd,
            "kind": np.asarray(kinds), "stat_keys": np.asarray(R.STAT_KEYS),
        }
        print(f"{name}: {len(recs)} levels, up to {cap} golds", flush=True)
    missing = [c for c in CASES if not seen.get(c)]
    assert not missing, f"no level shows: {missing}"
    os.makedirs(OUT, exist_ok=True)
    for name, arrays in files.items():
        path = os.path.join(OUT, name + ".npz")
        write_npz(path, arrays)
        size = os.path.getsize(path)
        assert size <= 100 * 1024, (path, size)
        total += size
    for c in CASES:
        print(f"{c}: {len(seen[c])} levels, e.g. {seen[c][0]}")
    print(f"unpatched engine on the 8 x 12 sets: identical, longest get_stats {rec.longest:.4f} s (the limit is 1 s)")
    print(total, "bytes in all")


if __name__ == "__main__":
    main()
