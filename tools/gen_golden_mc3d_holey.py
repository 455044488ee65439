"""Records the fixtures of the 3-D holey dungeon and maze (tests/golden/mc3d_holey/*.npz) from the reference.

The reference cannot construct either problem (Minecraft3DholeymazeProblem.__init__ calls Minecraft3DmazeProblem.__init__
without cfg), but get_stats runs on an instance made with __new__ and given its plain attributes: the dungeon needs _passable,
entrance_coords and exit_coords; the maze path_coords = [], render = False, entrance_coords and exit_coords.  The maze's
get_stats returns as path-length the length of the PREVIOUS call's path_coords, so it is called twice on each map and the second
answer is recorded: the value of the current map, which is what the device returns.  The loss is not recorded: its tables come
from __init__, so tests/mc3d_holey_rules.py pins it alone.

Recorded per level: the interior, the holes, the statistics, both ordered routes, the two legs' lengths (dungeon) and both
remove_stacked_path_tiles sets (sorted: the reference's lists are unordered); and gen_all_holes' list and the fixed holes for
two small shapes.  Data only; a rerun writes the same bytes.  Nothing is written unless the rules reproduce every recorded
field, every named case is present and every wrong rule fails at least one fixture.

    python tools/gen_golden_mc3d_holey.py            # needs the reference tree (oracle/ref_env.py)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import mc3d_holey_levels as Lv  # noqa: E402
import mc3d_holey_rules as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mc3d_holey")
NAMES = ["AIR", "DIRT", "CHEST", "SKULL", "PUMPKIN"]
HOLE_SHAPES = [(3, 3, 3), (3, 4, 5)]
MAX_FILE = 100 * 1024


def reference_level(problem, grid, holes):
    """get_stats of the reference on the bordered map, and what it leaves on the instance"""
    from control_pcgrl.envs.probs.minecraft.minecraft_3D_holey_dungeon_prob import Minecraft3DholeyDungeonProblem
    from control_pcgrl.envs.probs.minecraft.minecraft_3D_holey_maze_prob import Minecraft3DholeymazeProblem
    m = R.bordered_map(grid, holes)
    smap = [[[NAMES[v] for v in row] for row in plane] for plane in m.tolist()]
    up = np.array([1, 0, 0])
    if problem == "dungeon":
        p = Minecraft3DholeyDungeonProblem.__new__(Minecraft3DholeyDungeonProblem)
        p._passable = {"AIR", "CHEST", "SKULL", "PUMPKIN"}
    else:
        p = Minecraft3DholeymazeProblem.__new__(Minecraft3DholeymazeProblem)
        p.path_coords, p.render = [], False
    p.entrance_coords = np.array([holes[0], holes[0] + up])
    p.exit_coords = np.array([holes[1], holes[1] + up])
    stats = p.get_stats(smap)
    if problem == "maze":
        stats = p.get_stats(smap)  # the second call returns the current map's path-length
    tup = lambda path: [tuple(int(v) for v in t) for t in path]  # noqa: E731
    rec = {"stats": [int(stats[k]) for k in R.STAT_KEYS[problem]]}
    if problem == "dungeon":
        has_chest = stats["chests"] > 0
        rec["route"] = tup(p.ordered_path) if has_chest else []
        rec["overlay"] = sorted(tup(p.path_coords)) if has_chest else []
        rec["route2"] = tup(p.ordered_e_path)
        rec["overlay2"] = sorted(tup(p.min_e_path))
    else:
        rec["route"] = tup(p.ordered_connected_path)
        rec["overlay"] = sorted(tup(p.connected_path_coords))
        rec["route2"] = tup(p.ordered_path)
        rec["overlay2"] = sorted(tup(p.path_coords))
    return rec


def agrees(rec, res):
    """the fields of a reference record against the rules' result"""
    return (rec["stats"] == res["stats"] and rec["route"] == res["route"] and rec["route2"] == res["route2"]
            and rec["overlay"] == sorted(res["overlay"]) and rec["overlay2"] == sorted(res["overlay2"]))


def face_of(foot, shape):
    Z, Y, X = shape
    z, y, x = (int(v) for v in foot)
    return "x0" if x == 0 else "x1" if x == X + 1 else "y0" if y == 0 else "y1"


def cases_of(problem, grid, holes, res):
    """the named cases a level shows"""
    out = set()
    shape = tuple(grid.shape)
    out.add("shape-%dx%dx%d" % shape)
    out.add("face-" + face_of(holes[0], shape))
    out.add("face-" + face_of(holes[1], shape))
    m = R.bordered_map(grid, holes)
    P = m != R.DIRT
    reached = Lv.connected(problem, res)
    kinds = res["kinds"]
    if reached:
        names = {0: "walk", 1: "step-down", 2: "step-up", 3: "jump-level", 4: "jump-up", 5: "jump-down"}
        if kinds and set(kinds) == {0}:
            out.add("walk-only")
        out.update(names[k] for k in kinds if k)
    else:
        out.add("exit-unreachable")
    if res["again"]:
        out.add("re-accepted")
    for h in range(2):
        z, y, x = (int(v) for v in holes[h])
        air = m == R.AIR
        seen, stack = {(z, y, x)}, [(z, y, x)]
        while stack and len(seen) <= 2:
            cz, cy, cx = stack.pop()
            for dz, dy, dx in ((0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)):
                a = (cz + dz, cy + dy, cx + dx)
                if all(0 <= a[i] < m.shape[i] for i in range(3)) and air[a] and a not in seen:
                    seen.add(a)
                    stack.append(a)
        if len(seen) == 2:
            out.add("isolated-hole")
    if problem == "dungeon":
        paths = res["paths"]
        chests, enemies = res["chests"], res["enemies"]
        if R.count_regions(m == R.AIR) > R.count_regions(P):
            out.add("items-split-air")
        if chests:
            cx, cy, cz = chests[0]
            if P[cz - 1][cy][cx] and P[cz + 1][cy][cx]:
                out.add("chest-no-floor")
            if not P[cz + 1][cy][cx]:
                out.add("chest-no-headroom")
            if chests[0] not in paths and any(c in paths for c in chests[1:]):
                out.add("first-chest-unreachable-later-reachable")
        for ex, ey, ez in enemies:
            if P[ez - 1][ey][ex]:
                out.add("enemy-mid-air")
        dists = sorted(len(paths[e]) for e in enemies if e in paths)
        if len(dists) >= 2 and dists[0] == dists[1]:
            out.add("two-enemies-equal")
        if res["stats"][4] == 2:
            out.add("enemy-adjacent")
    return out


NEEDED = {
    "dungeon": {"walk-only", "step-up", "step-down", "jump-level", "jump-up", "jump-down", "re-accepted", "chest-no-floor",
                "chest-no-headroom", "first-chest-unreachable-later-reachable", "enemy-mid-air", "two-enemies-equal",
                "enemy-adjacent", "exit-unreachable", "face-x0", "face-x1", "face-y0", "face-y1", "isolated-hole",
                "items-split-air", "shape-3x3x3", "shape-3x4x5", "shape-7x7x7", "shape-15x15x15", "shape-16x16x16"},
    "maze": {"walk-only", "step-up", "step-down", "jump-level", "jump-up", "jump-down", "re-accepted", "exit-unreachable",
             "face-x0", "face-x1", "face-y0", "face-y1", "isolated-hole", "shape-3x3x3", "shape-3x4x5", "shape-7x7x7",
             "shape-15x15x15", "shape-16x16x16"},
}


def choose_levels(problem):
    """the hand-built levels, then from a pool of generated ones the first to show each case not yet shown, then one 15^3 and
    one 16^3 level that connects"""
    levels, shown = [], set()

    def take(name, grid, holes):
        res = R.evaluate(problem, grid, holes)
        got = cases_of(problem, grid, holes, res)
        levels.append((name, np.asarray(grid, dtype=np.uint8), np.asarray(holes, dtype=np.int32)))
        shown.update(got)

    for name, grid, holes in Lv.hand_levels(problem):
        take(name, grid, holes)
    for si, shape in enumerate([(3, 3, 3), (3, 4, 5), (7, 7, 7)]):
        for kind, (grids, holes) in (("terrain", Lv.structured_set(problem, shape, 160, seed=3600 + si)),
                                     ("random", Lv.random_set(problem, shape, 12, seed=3650 + si))):
            kept = 0
            for i in range(len(grids)):
                res = R.evaluate(problem, grids[i], holes[i])
                new = (cases_of(problem, grids[i], holes[i], res) & NEEDED[problem]) - shown
                if new or (kind == "random" and kept < 2) or (kind == "terrain" and kept < 4 and Lv.connected(problem, res)):
                    take("%s-%dx%dx%d-%d" % ((kind,) + shape + (i,)), grids[i], holes[i])
                    kept += 1
    for si, shape in enumerate([(15, 15, 15), (16, 16, 16)]):
        grids, holes = Lv.structured_set(problem, shape, 12, seed=3690 + si)
        for i in range(len(grids)):
            if Lv.connected(problem, R.evaluate(problem, grids[i], holes[i])):
                take("terrain-%dx%dx%d-%d" % (shape + (i,)), grids[i], holes[i])
                break
    return levels, shown


def flat(lists, width=3):
    """a list of lists of tuples as one int16 array and its int32 offsets"""
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(v) for v in lists])
    data = np.array([t for v in lists for t in v], dtype=np.int16).reshape(-1, width)
    return data, off


def main():
    import ref_env
    if not ref_env.available():
        raise SystemExit("the reference tree is not present: nothing recorded")
    files = {}
    for problem in ("dungeon", "maze"):
        levels, shown = choose_levels(problem)
        missing = NEEDED[problem] - shown
        if missing:
            raise SystemExit(f"{problem}: no level shows {sorted(missing)}: nothing written")
        recs, wrong = [], dict.fromkeys(name for name, _ in R.WRONG_RULES)
        for name, grid, holes in levels:
            rec = reference_level(problem, grid, holes)
            res = R.evaluate(problem, grid, holes)
            if not agrees(rec, res):
                raise SystemExit(f"{problem} {name}: the rules do not reproduce the reference "
                                 f"({rec['stats']} against {res['stats']}): nothing written")
            rec["leg_len"] = res["leg_len"]  # the two lists the reference concatenates; their sum is checked above
            for wname, kw in R.WRONG_RULES:
                if not agrees(rec, R.evaluate(problem, grid, holes, **kw)):
                    wrong[wname] = True
            recs.append(rec)
        files[problem] = (levels, recs, wrong)
        print(f"{problem}: {len(levels)} levels, cases {len(shown & NEEDED[problem])}/{len(NEEDED[problem])}", flush=True)
    unseen = [w for w, _ in R.WRONG_RULES if not any(files[p][2][w] for p in files)]
    if unseen:
        raise SystemExit(f"no fixture fails under the wrong rules {unseen}: nothing written")

    from control_pcgrl.envs.probs.minecraft.minecraft_3D_holey_maze_prob import Minecraft3DholeymazeProblem
    hole_lists = {}
    for shape in HOLE_SHAPES:
        p = Minecraft3DholeymazeProblem.__new__(Minecraft3DholeymazeProblem)
        p._height, p._width, p._length = shape
        p._border_idxs = p.get_border_idxs()
        p._hole_queue, p.fixed_holes = [], True
        pairs = np.array([[a[0], b[0]] for a, b in p.gen_all_holes()], dtype=np.int16)
        ent, ext = p.gen_holes()
        fixed = np.array([ent[0], ext[0]], dtype=np.int16)
        if not (np.array_equal(pairs, R.all_holes(shape)) and np.array_equal(fixed, R.fixed_holes(shape))):
            raise SystemExit(f"the rules' holes differ from the reference's at {shape}: nothing written")
        key = "%dx%dx%d" % shape
        hole_lists["all_holes_" + key], hole_lists["fixed_holes_" + key] = pairs, fixed

    os.makedirs(OUT, exist_ok=True)
    for problem, (levels, recs, _) in files.items():
        z = {"names": np.array([n for n, _, _ in levels]),
             "shapes": np.array([g.shape for _, g, _ in levels], dtype=np.int32),
             "holes": np.stack([h for _, _, h in levels]).astype(np.int32),
             "grids": np.concatenate([g.reshape(-1) for _, g, _ in levels]).astype(np.uint8),
             "stats": np.array([r["stats"] for r in recs], dtype=np.int32),
             "leg_len": np.array([r["leg_len"] for r in recs], dtype=np.int32)}
        for k in ("route", "route2", "overlay", "overlay2"):
            z[k], z[k + "_off"] = flat([r[k] for r in recs])
        if problem == "maze":
            z.update(hole_lists)
        path = os.path.join(OUT, problem + ".npz")
        np.savez_compressed(path, **z)
        size = os.path.getsize(path)
        assert size <= MAX_FILE, (path, size)
        print(f"{os.path.basename(path)}: {size} bytes", flush=True)


if __name__ == "__main__":
    main()
