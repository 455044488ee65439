"""The routes behind a Lode Runner level's path-length, recorded from the REFERENCE on the CPU ->
tests/golden/loderunner_routes/*.npz.  Data only; needs the reference tree; a few minutes on one core (the 16 x 32 levels take
most of it).  Not for the GPU machine.

    python tools/gen_golden_loderunner_routes.py

find_all_golds (loderunner/engine.py:281-308) calls Node.get_path on both goal nodes of every gold that counts: to_goal (landing
cell -> gold) and to_start (gold -> landing cell).  tools/gen_golden_loderunner.py's Recorder wraps that call, with the engine's
clock stopped as there; this script writes what it holds.  Per set (one file: a map shape) and per level:
  grids         uint8 [n][H][W]
  kind          which generator made the level
  pair_level    int32 [P], pair_gold int32 [P]: per counted gold, in call order, its level and its row-major gold index
  path_off      int32 [2 P + 1] into path_cells int16 [T][2]: get_path()[0] of to_goal (path 2 p) and of to_start (2 p + 1) as
                the reference lists it -- from the goal node back to the root, (row, column)
  act_off       int32 [2 P + 1] into path_actions int16 [T - 2 P]: Node.action from the goal node back, as an index into
                move_names (left right up down d-left d-right)

The script refuses to write unless tests/loderunner_rules.py's play(m, record=...) reproduces every list and the sets hold each
of CASES.  Files are written with fixed zip timestamps, so a rerun is byte-identical.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_golden_loderunner as G  # noqa: E402
import loderunner_levels as ll  # noqa: E402
import loderunner_routes_expect as X  # noqa: E402
import loderunner_rules as R  # noqa: E402
import ref_env  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "loderunner_routes")
# name: (H, W, [(kind, seed, n), ...]); "gold32": the first n gold-kind levels of the stream with a counted gold at index >= 32
SETS = {
    "stock_gold": (8, 12, [("gold", 3, 24), ("gold32", 1, 4)]),
    "stock_mixed": (8, 12, [("structured", 4, 32), ("random", 1, 24), ("detour", 26, 4)]),
    "h1w5": (1, 5, [("random", 11, 12), ("gold", 13, 12)]),
    "h2w1": (2, 1, [("random", 8, 6), ("gold", 10, 6)]),
    "h4w4": (4, 4, [("random", 14, 16), ("gold", 15, 16), ("structured", 16, 16)]),
    "h5w7": (5, 7, [("random", 17, 16), ("gold", 18, 16), ("structured", 19, 16)]),
    "h16w32": (16, 32, [("structured", 25, 4), ("gold", 24, 2), ("serpentine", 0, 1)]),
}
SHAPES = {(1, 5), (2, 1), (4, 4), (5, 7), (8, 12), (16, 32)}
CASES = (["a counted gold at index 32 or higher", "a state-2 gold in the round of the gold that found it",
          "gold reached with no way back", "return route not the reversed outward route"]
         + ["move " + n for n in R.MOVE_NAMES]
         + ["route longer than the BFS distance", "route of more than 64 cells", "16 x 32: route through a cell at index 256 or higher"])


def make_levels(kind, seed, n, h, w):
    if kind == "serpentine":
        return np.stack([X.serpentine(h, w)] * n)
    if kind == "gold32":
        rng, out = np.random.default_rng(seed), []
        while len(out) < n:
            m = ll.gold_level(rng, h, w)
            if any(j >= 32 for j, _, _ in X.pairs_of_rules(m)):
                out.append(m)
        return np.stack(out)
    return G.make_levels(kind, seed, n, h, w)


def recorded_pairs(m, rec):
    """the Recorder's get_path calls of one level as pairs (gold index, to_goal, to_start), moves as numbers"""
    golds = [(int(r), int(c)) for r, c in np.argwhere(m == R.GOLD)]
    paths = rec["paths"]
    assert len(paths) % 2 == 0
    out = []
    for k in range(0, len(paths), 2):
        both = []
        for cell, path, _, actions in paths[k:k + 2]:
            cells = [(int(r), int(c)) for r, c in path]
            assert cells[0] == cell and len(actions) == len(cells) - 1
            both.append((cells, [R.MOVE_NAMES.index(a) for a in actions]))
        gold = paths[k][0]
        assert both[1][0][-1] == gold and both[0][0][-1] == both[1][0][0] == tuple(rec["landing"])
        out.append((golds.index(gold), both[0], both[1]))
    return out


def cases_of(m, rec, pairs):
    got = set()
    H, W = m.shape
    if not pairs and not rec["runs"]:
        return got
    landing = tuple(rec["landing"])
    played = R.clean(m)
    played[landing] = R.EMPTY
    golds = [(int(r), int(c)) for r, c in np.argwhere(m == R.GOLD)]
    by_pair = {(src, goal): node for src, goal, node in rec["runs"]}
    for (src, goal), node in by_pair.items():
        if src == landing and node is not None and by_pair.get((goal, src), 0) is None:
            got.add("gold reached with no way back")
    found = {g for g, s in zip(golds, rec["state"]) if s == R.ON_THE_FALL}
    for j, to_goal, to_start in pairs:
        if j >= 32:
            got.add("a counted gold at index 32 or higher")
        if to_start[0] != to_goal[0][::-1]:
            got.add("return route not the reversed outward route")
        found.add(golds[j])
        for cells, moves in (to_goal, to_start):
            for a in moves:
                got.add("move " + R.MOVE_NAMES[a])
            if len(cells) - 1 > G.bfs_steps(played, cells[-1], cells[0]):
                got.add("route longer than the BFS distance")
            if len(cells) > 64:
                got.add("route of more than 64 cells")
            if (H, W) == (16, 32) and any(r * W + c >= 256 for r, c in cells):
                got.add("16 x 32: route through a cell at index 256 or higher")
            for p in cells[1:]:
                if played[p] == R.GOLD and p not in found:
                    found.add(p)
                    if golds.index(p) > j and golds.index(p) // 32 == j // 32:  # the device ran its searches in that round
                        got.add("a state-2 gold in the round of the gold that found it")
    return got


def main():
    assert ref_env.available(), "the reference tree is needed"
    assert {(h, w) for h, w, _ in SETS.values()} == SHAPES
    rec = G.Recorder()
    seen, files, total = {}, {}, 0
    for name, (h, w, parts) in SETS.items():
        grids, kinds, per_level = [], [], []
        for kind, seed, n in parts:
            for i, m in enumerate(make_levels(kind, seed, n, h, w)):
                r = rec.level(m, also_unpatched=False)
                G.check_rules(m, r, (name, kind, seed, i))
                pairs = recorded_pairs(m, r)
                assert pairs == X.pairs_of_rules(m), (name, kind, seed, i)  # play(m, record=...) reproduces every list
                assert [j for j, _, _ in pairs] == [j for j, s in enumerate(r["state"]) if s == R.BY_OWN_SEARCHES]
                assert [len(a[0]) for _, a, _ in pairs] == [d for d, s in zip(r["dist"], r["state"]) if s == R.BY_OWN_SEARCHES]
                for c in cases_of(m, r, pairs):
                    seen.setdefault(c, []).append(f"{name}:{kind}{seed}#{i}")
                grids.append(m)
                kinds.append(kind)
                per_level.append(pairs)
        pair_level, pair_gold, cells, actions, path_off, act_off = [], [], [], [], [0], [0]
        for i, pairs in enumerate(per_level):
            for j, to_goal, to_start in pairs:
                pair_level.append(i)
                pair_gold.append(j)
                for path, moves in (to_goal, to_start):
                    cells += path
                    actions += moves
                    path_off.append(len(cells))
                    act_off.append(len(actions))
        files[name] = {
            "grids": np.stack(grids).astype(np.uint8), "kind": np.asarray(kinds), "move_names": np.asarray(R.MOVE_NAMES),
            "pair_level": np.asarray(pair_level, dtype=np.int32), "pair_gold": np.asarray(pair_gold, dtype=np.int32),
            "path_off": np.asarray(path_off, dtype=np.int32), "path_cells": np.asarray(cells, dtype=np.int16).reshape(-1, 2),
            "act_off": np.asarray(act_off, dtype=np.int32), "path_actions": np.asarray(actions, dtype=np.int16),
        }
        for i, pairs in enumerate(per_level):  # what is written reads back as what was recorded
            assert X.pairs_of_fixture(files[name], i) == pairs
        print(f"{name}: {len(grids)} levels, {len(pair_level)} counted golds, {len(cells)} cells", flush=True)
    missing = [c for c in CASES if not seen.get(c)]
    assert not missing, f"no level shows: {missing}"
    os.makedirs(OUT, exist_ok=True)
    for name, arrays in files.items():
        path = os.path.join(OUT, name + ".npz")
        G.write_npz(path, arrays)
        size = os.path.getsize(path)
        assert size <= 100 * 1024, (path, size)
        total += size
    for c in CASES:
        print(f"{c}: {len(seen[c])} levels, e.g. {seen[c][0]}")
    print(total, "bytes in all")


if __name__ == "__main__":
    main()
