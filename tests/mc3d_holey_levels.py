"""Levels for the 3-D holey dungeon and maze tests, tools and fixtures: random maps almost never connect the two holes, so the
levels here are terrains -- a DIRT floor of varying height under AIR, with steps of one (walkable), cliffs (not), pits (a jump
over a one-tile gap) and ceilings -- between holes whose neighbourhood is levelled to them, plus items on the ground, in
mid-air and buried; and hand-built levels for what a generator rarely makes.  Plain numpy; deterministic for a seed."""
import functools

import numpy as np

import mc3d_holey_rules as R

AIR, DIRT, CHEST, SKULL, PUMPKIN = R.AIR, R.DIRT, R.CHEST, R.SKULL, R.PUMPKIN


@functools.lru_cache(maxsize=None)
def _border_cells(shape):
    Z, Y, X = shape
    d = np.zeros((Z + 2, Y + 2, X + 2), dtype=np.uint8)
    d[1:-2, 1:-1, 0] = d[1:-2, 1:-1, -1] = d[1:-2, 0, 1:-1] = d[1:-2, -1, 1:-1] = 1
    return np.argwhere(d == 1).astype(np.int32)


def face_holes(shape, rng):
    """a random pair of valid holes (one of gen_all_holes' pairs, drawn by rejection)"""
    idx = _border_cells(tuple(int(s) for s in shape))
    while True:
        a, b = idx[int(rng.integers(len(idx)))], idx[int(rng.integers(len(idx)))]
        if max(np.abs(a - b).max(), np.abs(a + np.array([1, 0, 0]) - b).max()) > 1:
            return np.stack([a, b]).astype(np.int32)


def _inward(foot, shape):
    """the interior column (iy, ix) next to a hole, interior indices"""
    Z, Y, X = shape
    z, y, x = (int(v) for v in foot)
    iy, ix = y - 1, x - 1
    if x == 0:
        ix = 0
    elif x == X + 1:
        ix = X - 1
    if y == 0:
        iy = 0
    elif y == Y + 1:
        iy = Y - 1
    return iy, ix


def terrain_level(rng, problem, shape, holes, rough=0.35, pits=0.12, ceilings=0.1, items=True):
    """One level: the heights run from the entrance's floor to the exit's with noise of one step, some pits and ceilings."""
    Z, Y, X = shape
    he, hx = int(holes[0][0]) - 1, int(holes[1][0]) - 1  # DIRT layers under each hole's foot
    (ey, ex), (xy, xx) = _inward(holes[0], shape), _inward(holes[1], shape)
    yy, xs = np.mgrid[0:Y, 0:X]
    de = np.abs(yy - ey) + np.abs(xs - ex)
    dx = np.abs(yy - xy) + np.abs(xs - xx)
    t = de / np.maximum(de + dx, 1)
    h = np.rint(he + (hx - he) * t).astype(np.int64)
    noise = rng.choice([-1, 0, 1], size=(Y, X), p=[rough / 2, 1 - rough, rough / 2])
    h = h + noise
    pit = rng.random((Y, X)) < pits
    h = np.where(pit, h - 3, h)
    h[ey, ex], h[xy, xx] = he, hx
    h = np.clip(h, 0, Z - 2)
    grid = np.full(shape, AIR, dtype=np.uint8)
    for z in range(Z):
        grid[z][h > z] = DIRT
    ceil = rng.random((Y, X)) < ceilings
    for y, x in np.argwhere(ceil):
        top = int(h[y, x]) + int(rng.integers(1, 4))
        if top < Z and (y, x) not in ((ey, ex), (xy, xx)):
            grid[top:, y, x] = DIRT
    if items and problem == "dungeon":
        n_items = int(rng.integers(1, 7))
        for k in range(n_items):
            y, x = int(rng.integers(Y)), int(rng.integers(X))
            where = rng.random()
            if k == 0:  # most levels get a chest on the ground, away from the columns inside the holes
                if (y, x) in ((ey, ex), (xy, xx)) or rng.random() < 0.1:
                    continue
                grid[int(h[y, x]), y, x] = CHEST
                continue
            z = int(h[y, x])
            if where < 0.2:
                z = min(Z - 1, z + int(rng.integers(1, 3)))  # in mid-air
            elif where < 0.3:
                z = max(0, z - 1)  # buried
            if z < Z:
                grid[z, y, x] = rng.choice([CHEST, SKULL, PUMPKIN], p=[0.4, 0.3, 0.3])
    return grid


def structured_set(problem, shape, count, seed, **kw):
    """count terrain levels with holes of their own: grids uint8 [count, Z, Y, X], holes int32 [count, 2, 3]"""
    rng = np.random.default_rng(seed)
    grids = np.empty((count,) + tuple(shape), dtype=np.uint8)
    holes = np.empty((count, 2, 3), dtype=np.int32)
    for i in range(count):
        holes[i] = face_holes(shape, rng) if i % 4 else R.fixed_holes(shape)
        grids[i] = terrain_level(rng, problem, shape, holes[i], **kw)
    return grids, holes


def random_set(problem, shape, count, seed):
    rng = np.random.default_rng(seed)
    p = [0.55, 0.3, 0.05, 0.05, 0.05] if problem == "dungeon" else [0.65, 0.35]
    grids = rng.choice(len(p), size=(count,) + tuple(shape), p=p).astype(np.uint8)
    holes = np.array([face_holes(shape, rng) for _ in range(count)], dtype=np.int32).reshape(count, 2, 3)
    return grids, holes


def connected(problem, res):
    """both legs reached (dungeon) or the exit connected (maze)"""
    if problem == "dungeon":
        return res["leg_len"][0] > 0 and res["leg_len"][1] > 0
    return res["stats"][2] > 0


def hand_levels(problem):
    """[(name, grid, holes)]: small levels built by hand for the cases a generator rarely makes"""
    out = []
    shape = (3, 4, 5)
    Z, Y, X = shape
    # a flat floor at the bottom: the entrance on the -x face, the exit on the +x face, both at z = 1
    flat = np.full(shape, AIR, dtype=np.uint8)
    holes_x = np.array([[1, 2, 0], [1, 3, X + 1]], dtype=np.int32)
    out.append(("flat-x-faces", flat.copy(), holes_x))
    holes_y = np.array([[1, 0, 2], [1, Y + 1, 4]], dtype=np.int32)
    out.append(("flat-y-faces", flat.copy(), holes_y))
    # the exit hole walled in: its two cells are a region of their own and the exit is not reached
    g = flat.copy()
    g[:, 2, X - 1] = DIRT  # the column inside the exit (3, X+1) -> interior (y 2, x X-1)
    out.append(("isolated-exit-hole", g, holes_x))
    # the entrance walled in as well: nothing but the hole is reached
    g2 = g.copy()
    g2[:, 1, 0] = DIRT
    out.append(("isolated-both-holes", g2, holes_x))
    if problem == "dungeon":
        g = flat.copy()
        g[0, 1, 0] = SKULL  # beside the entrance foot: the path is two tiles
        out.append(("enemy-adjacent", g, holes_x))
        g = flat.copy()
        g[0, 0, 1] = SKULL
        g[0, 2, 1] = PUMPKIN  # both two steps from the cell inside the entrance: equal distance, the SKULL first
        g[0, 1, 3] = CHEST
        out.append(("two-enemies-equal", g, holes_x))
        g = flat.copy()
        g[1, 1, 2] = CHEST  # floating: nobody can stand there, yet the second search starts on it
        g[1, 2, 3] = SKULL  # in mid-air
        out.append(("chest-midair", g, holes_x))
        g = flat.copy()
        g[0, 1, 2] = CHEST
        g[1, 1, 2] = DIRT  # no head-room
        g[0, 2, 2] = CHEST  # a later chest that is reachable: it does not count
        out.append(("chest-no-headroom", g, holes_x))
        g = flat.copy()
        g[0, 0, 4] = CHEST
        g[0, 0, 3] = g[1, 0, 3] = g[2, 0, 3] = DIRT
        g[0, 1, 4] = g[1, 1, 4] = g[2, 1, 4] = DIRT  # the first chest walled off
        g[0, 3, 1] = CHEST
        out.append(("first-chest-walled", g, holes_x))
        g = np.full(shape, DIRT, dtype=np.uint8)
        g[0:2, 1, :] = AIR
        g[0, 1, 2] = CHEST  # the chest splits the corridor's AIR in two
        g[1, 1, 2] = SKULL
        out.append(("items-split-air", g, np.array([[1, 2, 0], [1, 2, X + 1]], dtype=np.int32)))
    return out
