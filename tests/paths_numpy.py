"""The path rules of include/pcgrl_amd_paths.h stated in numpy (written for the tests, not taken from the reference): what
tests/test_paths_cpu.py replays against the fixtures recorded from the reference, and what tests/test_gpu_paths.py holds
fresh random maps against.  Cells are (row, col).  The keyword switches select the OTHER choice at each tie the rules settle;
tools/gen_golden_paths.py uses them to check that the fixtures tell the choices apart."""
import numpy as np

UP_LEFT_RIGHT_DOWN = ((-1, 0), (0, -1), (0, 1), (1, 0))
EMPTY, SOLID, PLAYER, KEY, DOOR = 0, 1, 2, 3, 4  # zelda tile ids (binary: 0 empty, 1 solid)


def bfs(passable, start):
    """4-neighbour distances from `start` inside `passable`, -1 where unreached"""
    d = np.full(passable.shape, -1, np.int32)
    front = np.zeros(passable.shape, bool)
    front[start] = passable[start]
    lev = 0
    while front.any():
        d[front] = lev
        nb = np.zeros_like(front)
        nb[1:] |= front[:-1]
        nb[:-1] |= front[1:]
        nb[:, 1:] |= front[:, :-1]
        nb[:, :-1] |= front[:, 1:]
        front = nb & passable & (d < 0)
        lev += 1
    return d


def trace(d, start, order=UP_LEFT_RIGHT_DOWN):
    """start, then the first neighbour in `order` one level below, down to level 0; empty if start is unreached"""
    if d[start] < 0:
        return []
    (r, c), path = start, [tuple(start)]
    while d[r, c] > 0:
        r, c = next((r + dr, c + dc) for dr, dc in order
                    if 0 <= r + dr < d.shape[0] and 0 <= c + dc < d.shape[1] and d[r + dr, c + dc] == d[r, c] - 1)
        path.append((r, c))
    return path


def binary_path(grid, order=UP_LEFT_RIGHT_DOWN, last_component=False, last_end=False):
    """-> (cells, L)"""
    passable, w = grid == EMPTY, grid.shape[1]
    seen, best_len, best = np.zeros(grid.shape, bool), 0, None
    for r, c in zip(*np.nonzero(passable)):  # the components in row-major order of their first cell
        if seen[r, c]:
            continue
        d0 = bfs(passable, (r, c))
        seen |= d0 >= 0
        d = bfs(passable, divmod(int(np.argmax(d0)), w))  # from the first farthest cell
        if d.max() > best_len or (last_component and d.max() == best_len):
            best_len, best = int(d.max()), d
    if best_len == 0:
        return [], 0
    ends = np.argwhere(best == best_len)
    return trace(best, tuple(int(v) for v in ends[-1 if last_end else 0]), order), best_len


def zelda_path(grid, order=UP_LEFT_RIGHT_DOWN):
    """-> cells"""
    spots = [np.argwhere(grid == t) for t in (PLAYER, KEY, DOOR)]
    if any(len(s) != 1 for s in spots):
        return []
    p, k, d = (tuple(int(v) for v in s[0]) for s in spots)
    a = trace(bfs((grid != SOLID) & (grid != DOOR), p), k, order)
    b = trace(bfs(grid != SOLID, k), d, order)
    return [cell for cell in a + b if cell not in (p, k, d)]


def path_of(problem, grid, **kw):
    return binary_path(grid, **kw)[0] if problem == "binary" else zelda_path(grid, **kw)


def as_arrays(paths, cap, shape):
    """a list of cell lists -> (coords int16 [n, cap, 2] with (-1, -1) fill, length int32 [n], overlay uint8 [n, H, W]):
    the layout of VecPcgrlEnv.paths"""
    n = len(paths)
    coords = np.full((n, cap, 2), -1, np.int16)
    length = np.array([len(p) for p in paths], np.int32)
    overlay = np.zeros((n,) + tuple(shape), np.uint8)
    for i, p in enumerate(paths):
        if p:
            a = np.asarray(p, np.int16)
            coords[i, :min(len(p), cap)] = a[:cap]
            overlay[i, a[:, 0], a[:, 1]] = 1
    return coords, length, overlay


def random_maps(problem, n, shape, rng):
    """maps of the fixtures' distribution: a solid density drawn uniformly per map, from [0, 1) for binary and from [0, 0.5)
    for zelda (above the percolation threshold hardly any key is reachable); zelda places the player, the key and the door
    each with probability 0.95 (a twentieth of those twice) and a few enemies"""
    h, w = shape
    grids = np.zeros((n, h, w), np.uint8)
    for g in grids:
        g[rng.random((h, w)) < rng.random() * (0.5 if problem == "zelda" else 1.0)] = SOLID
        if problem == "zelda":
            for tile in (PLAYER, KEY, DOOR):
                for _ in range(int(rng.random() < 0.95) + int(rng.random() < 0.05)):
                    g[rng.integers(h), rng.integers(w)] = tile
            for _ in range(int(rng.integers(0, 4))):
                if h * w > 4:
                    g[rng.integers(h), rng.integers(w)] = rng.integers(5, 8)
    return grids
