"""Solution paths of binary and zelda maps, recorded from the REFERENCE's own functions on the CPU (through oracle/ref_env.py)
-> tests/golden/paths/{binary,zelda}_<H>x<W>.npz.

    python tools/gen_golden_paths.py            # everything (needs the reference tree; about a minute)
    python tools/gen_golden_paths.py structured # only the structured set (below)

binary: helper.calc_longest_path(map, locations, ["empty"], get_path=True), what BinaryProblem.get_stats keeps as path_coords.
zelda:  ZeldaCtrlProblem(cfg).get_stats(map) with render_path = True, what it keeps as .path.

The files live in a sub-folder of tests/golden/ because other tests collect tests/golden/*.npz by pattern.  Layout: `grids`
uint8 [n, H, W]; the ragged paths as `cells` int16 [total, 2] (row, col) with `offsets` int32 [n + 1]; binary: `L` int32 [n],
the path-length statistic.  Every file starts with the hand-built maps (`n_hand` of them), random maps follow.

A second, STRUCTURED set goes to tests/golden/paths/structured/ (a folder of its own, so that the paths/*.npz patterns do not
see it): the same layout without n_hand, plus `names`, one family name per map.  Only hand-built maps, one shape per kernel
form, an odd shape and the largest (STRUCTURED_SHAPES): the long paths, the tied components and routes and the one- and
two-cell maps that random maps do not produce (structured_binary), and for zelda the key and the door at every distance
1..7 from the player, both halves on a serpentine -- 3 116 cells at 64 x 64, with the player's cell walked twice -- and
halves that are empty or share cells (structured_zelda).  The longest KNOWN binary path at 64 x 64 is the one-cell-wide
spiral's, 2 111 cells (the serpentine has 2 080); the bound on a binary path is n_cells.

The script fails unless the set tells the rules' tie-breaks apart (see check_worth): the fixtures are only worth replaying if
another neighbour order, another choice among tied components or among tied end cells would fail them.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import paths_numpy as pn  # noqa: E402
import ref_env  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "paths")
# one shape per kernel family (lanes per map x mask width), then the edges
SHAPES = [(8, 8), (5, 40), (16, 16), (12, 40), (24, 20), (20, 40), (40, 24), (40, 48),
          (1, 1), (1, 5), (5, 1), (7, 11), (32, 32), (64, 64)]
N_RANDOM = {(16, 16): 200, (8, 8): 200, (64, 64): 12}
TILES = {"binary": ["empty", "solid"],
         "zelda": ["empty", "solid", "player", "key", "door", "bat", "scorpion", "spider"]}


def serpentine(h, w):
    """one corridor through the whole map: the even rows, joined at alternating ends (64 x 64: 2 080 cells)"""
    g = np.ones((h, w), np.uint8)
    g[0::2] = 0
    for r in range(1, h, 2):
        g[r, w - 1 if (r // 2) % 2 == 0 else 0] = 0
    return g


def two_equal_components(h, w):
    """two open halves of the same size behind a solid line (None where the shape has no room)"""
    g = np.zeros((h, w), np.uint8)
    if w >= 3:
        g[:, w // 2] = 1
        if w % 2 == 0:
            g[:, 0] = 1
        return g
    if h >= 3:
        g[h // 2, :] = 1
        if h % 2 == 0:
            g[0, :] = 1
        return g
    return None


def hand_maps(problem, shape):
    h, w = shape
    maps = [np.zeros(shape, np.uint8), np.ones(shape, np.uint8)]
    if shape in ((16, 16), (64, 64)):
        maps.append(serpentine(h, w))
    t = two_equal_components(h, w)
    if t is not None:
        maps.append(t)
    if problem == "zelda":
        if h >= 3 and w >= 3:
            for walled in (pn.KEY, pn.DOOR):  # the key / the door behind four solid cells
                g = np.zeros(shape, np.uint8)
                g[0, 0], g[h - 1, w - 1], g[h - 1, 0] = pn.PLAYER, (pn.DOOR if walled == pn.KEY else pn.KEY), 0
                r, c = h // 2, w // 2
                g[r, c] = walled
                for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                    g[rr, cc] = pn.SOLID
                if g[0, 0] == pn.PLAYER and (g == pn.KEY).sum() == 1 and (g == pn.DOOR).sum() == 1:
                    maps.append(g)
        if w >= 5:
            g = np.ones(shape, np.uint8)  # a corridor key . player . door: the way from the key to the door crosses the player
            g[0, :5] = (pn.KEY, pn.EMPTY, pn.PLAYER, pn.EMPTY, pn.DOOR)
            maps.append(g)
            g = np.zeros(shape, np.uint8)  # two players
            g[0, :5] = (pn.PLAYER, pn.KEY, pn.EMPTY, pn.DOOR, pn.PLAYER)
            maps.append(g)
            g = np.zeros(shape, np.uint8)  # an open map with one of each
            g[0, 0], g[h - 1, w - 1], g[0, w - 1] = pn.PLAYER, pn.KEY, pn.DOOR
            maps.append(g)
    return maps


def reference_paths(problem, shape, grids):
    """-> (list of [len, 2] int arrays (row, col), list of path-length statistics)"""
    from control_pcgrl.envs.helper import calc_longest_path, get_string_map, get_tile_locations
    paths, lens = [], []
    prob = None
    if problem == "zelda":
        from control_pcgrl.envs.probs.zelda.zelda_ctrl_prob import ZeldaCtrlProblem
        prob = ZeldaCtrlProblem(ref_env.make_cfg("zelda", "narrow", shape))
        prob.render_path = True
    for g in grids:
        m = get_string_map(g, TILES[problem])
        if problem == "binary":
            length, path = calc_longest_path(m, get_tile_locations(m, TILES[problem]), ["empty"], get_path=True)
        else:
            length, path = prob.get_stats(m)["path-length"], prob.path
        paths.append(np.asarray(path, np.int64).reshape(-1, 2))
        lens.append(int(length))
    return paths, lens


def check_worth(problem, shape, grids, paths):
    """the properties that make the set worth replaying, on the shapes that carry 200 random maps"""
    if shape not in ((16, 16), (8, 8)):
        return
    n = len(grids)
    nonempty = sum(len(p) > 0 for p in paths)
    same = lambda a, b: len(a) == len(b) and all(tuple(x) == tuple(y) for x, y in zip(a, b))  # noqa: E731
    if problem == "zelda":
        print(f"  zelda {shape}: {nonempty} of {n} paths non-empty")
        if shape == (16, 16):
            assert 3 * nonempty >= n, "zelda 16x16: fewer than a third of the paths are non-empty"
        return
    assert 2 * nonempty >= n, f"binary {shape}: fewer than half of the paths are non-empty"
    if shape != (16, 16):
        return
    rev = sum(not same(pn.binary_path(g, order=pn.UP_LEFT_RIGHT_DOWN[::-1])[0], p) for g, p in zip(grids, paths))
    comp = sum(not same(pn.binary_path(g, last_component=True)[0], p) for g, p in zip(grids, paths))
    end = sum(not same(pn.binary_path(g, last_end=True)[0], p) for g, p in zip(grids, paths))
    print(f"  binary {shape}: {nonempty} of {n} non-empty; another path with the reversed neighbour order in {rev}, the last "
          f"tied component in {comp}, the last tied end cell in {end}")
    assert rev >= 20 and comp >= 5 and end >= 5, "the fixtures do not tell the tie-breaks apart"


STRUCTURED_OUT = os.path.join(OUT, "structured")
# one shape per kernel form (lanes per map / mask bits: 8/32, 16/32, 32/32, 64/32, 32/64, 64/64), an odd one, the largest
STRUCTURED_SHAPES = [(8, 8), (5, 7), (16, 16), (20, 24), (40, 16), (12, 40), (40, 48), (64, 64)]


def spiral(h, w):
    """a one-cell-wide corridor wound inwards from (0, 0), one solid cell between its turns (64 x 64: 2 111 cells)"""
    g = np.ones((h, w), np.uint8)
    r, c, k = 0, 0, 0
    g[0, 0] = 0
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def free(rr, cc):  # inside, solid, and touching no open cell but the one we come from
        if not (0 <= rr < h and 0 <= cc < w) or g[rr, cc] == 0:
            return False
        return all((ar, ac) == (r, c) or not (0 <= ar < h and 0 <= ac < w) or g[ar, ac] == 1
                   for ar, ac in ((rr - 1, cc), (rr + 1, cc), (rr, cc - 1), (rr, cc + 1)))

    while True:
        for turn in (0, 1):
            dr, dc = dirs[(k + turn) % 4]
            if free(r + dr, c + dc):
                k, r, c = (k + turn) % 4, r + dr, c + dc
                g[r, c] = 0
                break
        else:
            return g


def corridor(g):
    """the cells of a one-corridor map in walking order from (0, 0)"""
    d = pn.bfs(g == 0, (0, 0))
    cells = np.argwhere(d >= 0)
    return [tuple(int(v) for v in cells[i]) for i in np.argsort(d[d >= 0], kind="stable")]


def structured_binary(shape):
    """-> [(family name, map)]"""
    h, w = shape
    rr, cc = np.mgrid[0:h, 0:w]
    solid = lambda: np.ones(shape, np.uint8)  # noqa: E731
    comb = solid()  # row 0 and the even columns open
    comb[0, :] = 0
    comb[:, 0::2] = 0
    rooms = np.zeros(shape, np.uint8)  # every fourth column solid: components that tie
    rooms[:, 3::4] = 1
    frame = solid()  # a cycle: routes that tie
    frame[0, :] = frame[h - 1, :] = 0
    frame[:, 0] = frame[:, w - 1] = 0
    stairs = ((cc != rr) & (cc != rr + 1)).astype(np.uint8)
    two, one = solid(), solid()
    two[h - 1, w - 2:] = 0
    one[h - 1, w - 1] = 0
    return [("spiral", spiral(h, w)), ("comb", comb), ("checkerboard", ((rr + cc) % 2).astype(np.uint8)),
            ("equal-rooms", rooms), ("open-frame", frame), ("staircase", stairs), ("two-cells-last-row", two),
            ("one-cell-last-corner", one), ("serpentine", serpentine(h, w)),
            ("serpentine-transposed", np.ascontiguousarray(serpentine(w, h).T))]


def structured_zelda(shape):
    """-> [(family name, map)]"""
    h, w = shape
    out = []
    # the key and the door side by side in row 0, the nearer one d cells from the player: every residue of the recorded
    # sweep's unrolling and its early stop; with the door in front the first half goes round it (open map) or does not exist
    # (rows 1.. solid)
    for ground in ("open", "row0"):
        for first in ("key", "door"):
            for d in range(1, 8):
                if d + 1 >= w:
                    continue
                g = np.zeros(shape, np.uint8)
                if ground == "row0":
                    g[1:] = pn.SOLID
                g[0, 0] = pn.PLAYER
                g[0, d], g[0, d + 1] = (pn.KEY, pn.DOOR) if first == "key" else (pn.DOOR, pn.KEY)
                out.append((f"{ground}-{first}-first-d{d}", g))
    for name, base in (("serpentine", serpentine(h, w)), ("serpentine-transposed", np.ascontiguousarray(serpentine(w, h).T))):
        way = corridor(base)
        g = base.copy()  # no door: no path
        g[way[0]], g[way[-1]] = pn.PLAYER, pn.KEY
        out.append((f"{name}-no-door", g))
        g = g.copy()  # the door in front of the player: only the half from the door to the key
        g[way[1]] = pn.DOOR
        out.append((f"{name}-door-second-cell", g))
        g = base.copy()  # both halves, the second one through the player's cell
        g[way[0]], g[way[len(way) // 2]], g[way[-1]] = pn.KEY, pn.PLAYER, pn.DOOR
        out.append((f"{name}-player-middle", g))
        g = g.copy()
        for i, cell in enumerate(way[2:-2:5]):
            if g[cell] == pn.EMPTY:
                g[cell] = 5 + i % 3
        out.append((f"{name}-player-middle-enemies", g))
    g = np.zeros(shape, np.uint8)  # the halves share cells
    g[0, 0], g[0, 1], g[h - 1, w - 1] = pn.PLAYER, pn.DOOR, pn.KEY
    out.append(("open-key-far-door-near", g))
    return out


def structured():
    os.makedirs(STRUCTURED_OUT, exist_ok=True)
    total = 0
    for problem, family in (("binary", structured_binary), ("zelda", structured_zelda)):
        for shape in STRUCTURED_SHAPES:
            named = family(shape)
            grids = np.array([g for _, g in named], np.uint8)
            paths, lens = reference_paths(problem, shape, grids)
            for g, p, length in zip(grids, paths, lens):  # the numpy rules reproduce every recorded path
                mine = pn.path_of(problem, g)
                assert len(mine) == len(p) and all(tuple(a) == tuple(b) for a, b in zip(mine, p)), (problem, shape, g, p, mine)
                assert problem != "binary" or len(p) == (length + 1 if length else 0)
            out = dict(grids=grids, offsets=np.cumsum([0] + [len(p) for p in paths]).astype(np.int32),
                       cells=np.concatenate(paths).astype(np.int16), names=np.array([name for name, _ in named]))
            if problem == "binary":
                out["L"] = np.array(lens, np.int32)
            path = os.path.join(STRUCTURED_OUT, f"{problem}_{shape[0]}x{shape[1]}.npz")
            np.savez_compressed(path, **out)
            total += os.path.getsize(path)
            print(f"{os.path.relpath(path, ROOT)}: {len(grids)} maps, longest path {max(len(p) for p in paths)}, "
                  f"{os.path.getsize(path)} bytes")
            assert os.path.getsize(path) <= 16 * 1024
    print("structured total", total, "bytes")
    assert total <= 100 * 1024


def main():
    assert ref_env.available(), "reference tree not present"
    if sys.argv[1:] == ["structured"]:
        return structured()
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for problem in ("binary", "zelda"):
        for k, shape in enumerate(SHAPES):
            rng = np.random.default_rng(1000 * (problem == "zelda") + k)
            hand = hand_maps(problem, shape)
            grids = np.concatenate((np.array(hand, np.uint8), pn.random_maps(problem, N_RANDOM.get(shape, 40), shape, rng)))
            paths, lens = reference_paths(problem, shape, grids)
            for g, p, length in zip(grids, paths, lens):  # the rules as the tests state them: agreement is checked here already
                mine = pn.path_of(problem, g)
                assert len(mine) == len(p) and all(tuple(a) == tuple(b) for a, b in zip(mine, p)), (problem, shape, g, p, mine)
                assert problem != "binary" or len(p) == (length + 1 if length else 0)
            check_worth(problem, shape, grids[len(hand):], paths[len(hand):])
            out = dict(grids=grids, n_hand=len(hand), offsets=np.cumsum([0] + [len(p) for p in paths]).astype(np.int32),
                       cells=np.concatenate(paths).astype(np.int16))
            if problem == "binary":
                out["L"] = np.array(lens, np.int32)
            path = os.path.join(OUT, f"{problem}_{shape[0]}x{shape[1]}.npz")
            np.savez_compressed(path, **out)
            total += os.path.getsize(path)
            print(f"{os.path.relpath(path, ROOT)}: {len(grids)} maps ({len(hand)} hand-built), longest path "
                  f"{max(len(p) for p in paths)}, {os.path.getsize(path)} bytes")
    print("total", total, "bytes")
    assert total < 300 * 1024
    structured()


if __name__ == "__main__":
    main()
