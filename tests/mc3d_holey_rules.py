"""The 3-D holey dungeon and maze of the reference, restated on integer maps: what
Minecraft3DholeyDungeonProblem.get_stats (probs/minecraft/minecraft_3D_holey_dungeon_prob.py:87-147) and
Minecraft3DholeymazeProblem.get_stats (probs/minecraft/minecraft_3D_holey_maze_prob.py:71-129) compute on the bordered map that
HoleyRepresentation3D hands them (reps/wrappers.py:182-185), with helper_3D.run_dijkstra (:422-490) and helper_3D._passable
(:214-319) written out as they stand -- path lists and all, no parent pointers: the device's parent chain is checked against
this, not against itself.  The loss is ControlWrapper.get_loss (control_wrappers.py:318-345) over the frozen tables.

Plain Python and numpy; no torch, no device.  `WRONG_RULES` are plausible mistakes: the recorder refuses to write fixtures
unless each of them fails at least one.
"""
import math
from collections import deque

import numpy as np

AIR, DIRT, CHEST, SKULL, PUMPKIN = 0, 1, 2, 3, 4
DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1))  # helper_3D.py:220
ERR_TILE, ERR_HOLE, ERR_QUEUE = 1, 2, 4
STAT_KEYS = {"dungeon": ["regions", "path-length", "chests", "enemies", "nearest-enemy", "n_jump"],
             "maze": ["regions", "path-length", "connected-path-length", "n_jump"]}
N_TILES = {"dungeon": 5, "maze": 2}
PLAY = 12

# the frozen 15^3 tables (minecraft_3D_maze_prob.py:33-35, :46-50): ceil(15 / 2) * 15 + floor(15 / 2) = 127 a floor, two passes
# over each of 15 // 3 floors
MAX_PATH = 2 * (15 // 3) * (math.ceil(15 / 2) * 15 + 15 // 2)  # 1270
TARGETS = {
    "dungeon": {"regions": 1, "path-length": 10 * MAX_PATH, "chests": 1, "enemies": (2, 5),
                "nearest-enemy": (5, MAX_PATH // 2), "n_jump": (2, 5)},
    "maze": {"regions": 1, "path-length": 10 * MAX_PATH, "connected-path-length": 10 * MAX_PATH, "n_jump": 5},
}
WEIGHTS = {
    "dungeon": {"regions": 0, "path-length": 100, "chests": 300, "enemies": 100, "nearest-enemy": 200, "n_jump": 100},
    "maze": {"regions": 0, "path-length": 100, "connected-path-length": 120, "n_jump": 150},
}
BOUNDS = {
    "dungeon": {"regions": (0, math.ceil(15 * 15 / 2 * 15)), "path-length": (0, MAX_PATH), "chests": (0, 15 ** 3 // 4),
                "enemies": (0, 15 ** 3 // 4), "nearest-enemy": (0, MAX_PATH // 2), "n_jump": (0, MAX_PATH // 2)},
    "maze": {"regions": (0, math.ceil(15 * 15 / 2 * 15)), "path-length": (0, MAX_PATH + 2),
             "connected-path-length": (0, MAX_PATH + 2), "n_jump": (0, MAX_PATH // 2)},
}


def hole_ok(foot, shape):
    """holey_prob_3D.py:28-31: a foot cell on one of the four side faces, off the edges, z in 1..Z-1 (bordered coordinates)"""
    Z, Y, X = shape
    z, y, x = (int(v) for v in foot)
    if not 1 <= z <= Z - 1:
        return False
    return ((x in (0, X + 1) and 1 <= y <= Y) or (y in (0, Y + 1) and 1 <= x <= X))


def fixed_holes(shape):
    """holey_prob_3D.py:73-76"""
    Z, Y, X = shape
    return np.array([[1, 0, X], [2, Y + 1, 1]], dtype=np.int32)


def all_holes(shape):
    """gen_all_holes (holey_prob_3D.py:35-39): every ordered pair of border cells whose exit foot is more than one cell away,
    in some axis, from the entrance's foot or head: int32 [pairs, 2, 3]"""
    Z, Y, X = shape
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
    return np.stack([a[ok], b[ok]], axis=1)


def bordered_map(grid, holes):
    """The map get_stats sees: a DIRT border all round, the four hole cells AIR"""
    grid = np.asarray(grid)
    Z, Y, X = grid.shape
    m = np.full((Z + 2, Y + 2, X + 2), DIRT, dtype=np.int64)
    m[1:-1, 1:-1, 1:-1] = grid
    for z, y, x in np.asarray(holes).reshape(2, 3):
        m[z][y][x] = AIR
        m[z + 1][y][x] = AIR
    return m


def passable_moves(P, x, y, z, n_j, dirs=DIRS):
    """helper_3D._passable (:214-319) on the boolean passable map P[z][y][x]: [((nx, ny, nz, n_j), traversed, kind)], the
    dict's insertion order.  kind: 0 walk, 1 step down, 2 step up, 3 / 4 / 5 jump landing level / up / down."""
    out = []
    nZ, nY, nX = len(P), len(P[0]), len(P[0][0])
    for dx, dy in dirs:
        nx, ny, nz = x + dx, y + dy, z
        jx, jy, jz = x + 2 * dx, y + 2 * dy, z
        if nx < 0 or ny < 0 or nx >= nX or ny >= nY:
            continue
        if (nz == 0 or (nz > 0 and not P[nz - 1][ny][nx])) and P[nz][ny][nx] and P[nz + 1][ny][nx]:
            out.append(((nx, ny, nz, n_j), [], 0))
        elif ((nz - 1 == 0 or (nz - 1 > 0 and not P[nz - 2][ny][nx])) and P[nz - 1][ny][nx] and P[nz][ny][nx]
              and P[nz + 1][ny][nx]):
            out.append(((nx, ny, nz - 1, n_j), [(nx, ny, nz)], 1))
        elif nz + 2 < nZ and not P[nz][ny][nx] and P[nz + 1][ny][nx] and P[nz + 2][ny][nx] and P[nz + 2][y][x]:
            out.append(((nx, ny, nz + 1, n_j), [(x, y, nz + 1)], 2))
        elif (nz - 2 >= 0 and nz + 2 < nZ and P[nz + 2][ny][nx] and P[nz + 1][ny][nx] and P[nz][ny][nx] and P[nz - 1][ny][nx]
              and P[nz - 2][ny][nx] and P[nz + 2][y][x] and 0 <= jx < nX and 0 <= jy < nY):
            if P[jz + 1][jy][jx] and P[jz + 2][jy][jx] and P[jz][jy][jx] and not P[jz - 1][jy][jx]:
                out.append(((jx, jy, jz, n_j + 1), [(nx, ny, nz)], 3))
            elif jz + 3 < nZ and P[jz + 3][jy][jx] and P[jz + 2][jy][jx] and P[jz + 1][jy][jx] and not P[jz][jy][jx]:
                out.append(((jx, jy, jz + 1, n_j + 1), [(nx, ny, nz), (nx, ny, nz + 1)], 4))
            elif P[jz][jy][jx] and P[jz + 1][jy][jx] and P[jz - 1][jy][jx] and not P[jz - 2][jy][jx]:
                out.append(((jx, jy, jz - 1, n_j + 1), [(nx, ny, nz), (nx, ny, nz - 1)], 5))
    return out


def run_search(P, x, y, z, dirs=DIRS):
    """helper_3D.run_dijkstra (:422-490): paths (a dict in order of first acceptance), jumps, and the counts of accepted pops
    and of queue entries made (the start included), whether some cell was accepted more than once, and the move kinds along
    each accepted path"""
    paths, jumps, kinds = {}, {}, {}
    queue = deque([(x, y, z, [(x, y, z)], 0, [])])
    accepted, pushed, again = 0, 1, False
    nZ = len(P)
    while queue:
        cx, cy, cz, path, n_jump, moves = queue.popleft()
        old = paths.get((cx, cy, cz), [])
        if len(old) > 0 and len(old) <= len(path):
            continue
        if cz + 1 == nZ or not P[cz + 1][cy][cx]:
            continue
        again = again or (cx, cy, cz) in paths
        paths[(cx, cy, cz)] = path
        jumps[(cx, cy, cz)] = n_jump
        kinds[(cx, cy, cz)] = moves
        accepted += 1
        for (nx, ny, nz, n_j), traversed, kind in passable_moves(P, cx, cy, cz, n_jump, dirs):
            queue.append((nx, ny, nz, path + traversed + [(nx, ny, nz)], n_j, moves + [kind]))
            pushed += 1
    return paths, jumps, accepted, pushed, again, kinds


def unstack(path):
    """remove_stacked_path_tiles (helper_3D.py:657-675) as a set: a tile leaves when the tile below it is in the path"""
    s = set(tuple(int(v) for v in e) for e in path)
    return {t for t in s if (t[0], t[1], t[2] - 1) not in s}


def tile_locations(m, tile):
    """get_tile_locations' list of one tile (helper_3D.py:22-30): (x, y, z) in z-major, y, x order"""
    return [(int(x), int(y), int(z)) for z, y, x in np.argwhere(m == tile)]


def count_regions(mask):
    """calc_num_regions (helper_3D.py:396-406): 6-neighbour regions of a boolean map"""
    mask = np.asarray(mask, dtype=bool)
    seen = np.zeros_like(mask)
    nZ, nY, nX = mask.shape
    regions = 0
    for z, y, x in np.argwhere(mask):
        if seen[z, y, x]:
            continue
        regions += 1
        seen[z, y, x] = True
        stack = [(int(z), int(y), int(x))]
        while stack:
            cz, cy, cx = stack.pop()
            for dz, dy, dx in ((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)):
                az, ay, ax = cz + dz, cy + dy, cx + dx
                if 0 <= az < nZ and 0 <= ay < nY and 0 <= ax < nX and mask[az, ay, ax] and not seen[az, ay, ax]:
                    seen[az, ay, ax] = True
                    stack.append((az, ay, ax))
    return regions


def target_term(value, trg, weight):
    """control_wrappers.py:337-342: one term, -(distance to the target or to the nearest integer of arange(lo, hi)) * weight"""
    if isinstance(trg, tuple):
        lo, hi = float(trg[0]), float(trg[0] + math.ceil(trg[1] - trg[0]) - 1)
        d = lo - value if value < lo else (value - hi if value > hi else 0.0)
    else:
        d = abs(float(trg) - value)
    return -float(d) * float(weight)


def loss_of(problem, stats):
    """get_loss with the statistics taken in STAT_KEYS order (the reference sums over a set; every term is an integer-valued
    double, so the order does not show): each term rounded to double, then added"""
    loss = 0.0
    for k, v in zip(STAT_KEYS[problem], stats):
        loss = loss + target_term(float(v), TARGETS[problem][k], WEIGHTS[problem][k])
    return loss


def evaluate(problem, grid, holes, regions_all_passable=False, nearest_le=False, chest_needs_standable=False,
             maze_len_raw=False, last_longest=False, dirs=DIRS):
    """One level.  Returns a dict: stats (STAT_KEYS order), loss, error, play (PLAY ints), route and route2 (lists of
    (x, y, z)), leg_len (dungeon), overlay and overlay2 (sets of (x, y, z)); and for choosing levels: kinds (the move kinds
    along the main route), again (the entrance search accepted a cell twice), paths (the entrance search's).  The keyword flags
    are WRONG_RULES' mistakes."""
    grid = np.asarray(grid)
    holes = np.asarray(holes).reshape(2, 3)
    nstat = len(STAT_KEYS[problem])
    error = 0
    if (grid >= N_TILES[problem]).any():
        error |= ERR_TILE
        grid = np.where(grid >= N_TILES[problem], DIRT, grid)
    res = {"route": [], "route2": [], "leg_len": [0, 0], "overlay": set(), "overlay2": set()}
    play = [0] * PLAY
    play[5:11] = [-1] * 6
    if not (hole_ok(holes[0], grid.shape) and hole_ok(holes[1], grid.shape)):
        res.update(stats=[-1] * nstat, loss=-math.inf, error=error | ERR_HOLE, play=play)
        return res
    m = bordered_map(grid, holes)
    P = (m != DIRT)
    regions = count_regions(P if regions_all_passable else m == AIR)
    pz, py, px = (int(v) for v in holes[0])
    ex, ey, ez = int(holes[1][2]), int(holes[1][1]), int(holes[1][0])
    P = P.tolist()
    if problem == "maze":
        paths, jumps, acc, pushed, again, kinds = run_search(P, px, py, pz, dirs)
        play[0], play[1], play[2] = 1, acc, pushed
        connected = paths.get((ex, ey, ez), [])
        n_jump = jumps.get((ex, ey, ez), 0)
        tiles = list(paths.items())  # never empty: the entrance has head-room
        lens = [len(p) for _, p in tiles]
        best = max(lens)
        at = (len(lens) - 1 - lens[::-1].index(best)) if last_longest else lens.index(best)
        far, longest = tiles[at]
        play[5:8] = list(far)
        path_length = len(longest) if maze_len_raw else len(unstack(longest))
        stats = [regions, path_length, len(connected) if connected else -1, n_jump]
        res.update(route=list(connected), route2=list(longest), overlay=unstack(connected), overlay2=unstack(longest),
                   kinds=list(kinds.get((ex, ey, ez), [])), again=again, paths=paths)
    else:
        chests = tile_locations(m, CHEST)
        enemies = tile_locations(m, SKULL) + tile_locations(m, PUMPKIN)
        stats = [regions, 0, len(chests), len(enemies), 0, 0]
        res.update(kinds=[], again=False, paths={}, chests=chests, enemies=enemies)
        if enemies or chests:
            paths, jumps, acc, pushed, again, kinds = run_search(P, px, py, pz, dirs)
            play[0], play[1], play[2] = 1, acc, pushed
            res.update(again=again, paths=paths)
        if enemies:
            min_dist, e_path, e_at = 0, [], None
            for e in enemies:
                p = paths.get(e, [])
                d = len(p)
                if d > 0 and ((d <= min_dist if nearest_le else d < min_dist) or min_dist == 0):
                    min_dist, e_path, e_at = d, p, e
            stats[4] = min_dist
            if e_at is not None:
                play[8:11] = list(e_at)
            res.update(route2=list(e_path), overlay2=unstack(e_path))
        if chests:
            c = chests[0]
            play[5:8] = list(c)
            path_c = paths.get(c, [])
            stats[1] += len(path_c)
            stats[5] += jumps.get(c, 0)
            standable = P[c[2] + 1][c[1]][c[0]] and not P[c[2] - 1][c[1]][c[0]]
            kinds_d = {}
            if chest_needs_standable and not standable:
                path_d = []
            else:
                paths_d, jumps_d, acc, pushed, _, kinds_d = run_search(P, c[0], c[1], c[2], dirs)
                play[0] |= 2
                play[3], play[4] = acc, pushed
                path_d = paths_d.get((ex, ey, ez), [])
                stats[5] += jumps_d.get((ex, ey, ez), 0)
            stats[1] += len(path_d)
            route = list(path_c) + list(path_d)
            res.update(route=route, leg_len=[len(path_c), len(path_d)], overlay=unstack(route),
                       kinds=list(kinds.get(c, [])) + list(kinds_d.get((ex, ey, ez), [])))
    res.update(stats=[int(v) for v in stats], loss=loss_of(problem, stats), error=error, play=play)
    return res


def reaccepts(problem, grid, holes):
    """whether the entrance search accepts some cell a second time (a named case of the fixtures)"""
    m = bordered_map(grid, holes)
    P = (m != DIRT).tolist() if problem == "dungeon" else (m == AIR).tolist()
    z, y, x = (int(v) for v in np.asarray(holes).reshape(2, 3)[0])
    return run_search(P, x, y, z)[4]


WRONG_RULES = [
    ("regions over every passable tile", {"regions_all_passable": True}),
    ("<= for the nearest enemy", {"nearest_le": True}),
    ("chest leg only from a standable chest", {"chest_needs_standable": True}),
    ("maze length before remove_stacked_path_tiles", {"maze_len_raw": True}),
    ("last instead of first longest path", {"last_longest": True}),
    ("direction order -x, -y, +x, +y", {"dirs": ((-1, 0), (0, -1), (1, 0), (0, 1))}),
]
