"""Dangerous Dave maps for the fixtures (tools/gen_golden_ddave.py) and the GPU tests: uint8 [H][W] of tile ids 0..6 (empty,
solid, player, exit, diamond, key, spike).  Every generator works at any shape from 1 x 1 and never leaves more than 64
diamonds on a map (the device's limit), so no generated level is left unsearched for that reason."""
import numpy as np

EMPTY, SOLID, PLAYER, EXIT, DIAMOND, KEY, SPIKE = range(7)
PROB = (0.5, 0.3, 0.02, 0.02, 0.04, 0.02, 0.1)  # probs/ddave/ddave_prob.py:19 _prob, in tile order
MAX_DIAMONDS = 64


def cap_diamonds(m):
    """the diamonds past the 64th in row-major order become empty"""
    at = np.flatnonzero(m.ravel() == DIAMOND)
    m.ravel()[at[MAX_DIAMONDS:]] = EMPTY
    return m


def place_one_each(rng, m, where=None):
    """exactly one player, exit and key, on distinct cells among `where` (flat indices; all cells by default): as many of the
    three as fit"""
    m[(m == PLAYER) | (m == EXIT) | (m == KEY)] = EMPTY
    cells = np.arange(m.size) if where is None else np.asarray(where)
    pick = rng.permutation(cells)[:3]
    for tile, at in zip((PLAYER, KEY, EXIT), pick):
        m.ravel()[at] = tile
    return m


def chance_level(rng, h, w, prob=PROB):
    """every cell from the tile probabilities: how many players, exits and keys there are is left to chance"""
    return cap_diamonds(rng.choice(7, size=(h, w), p=prob).astype(np.uint8))


def random_level(rng, h, w, solid=0.3, diamond=0.04, spike=0.1):
    """the other tiles from their probabilities, then one player, one key and one exit"""
    p = np.array([0, solid, 0, 0, diamond, 0, spike], float)
    p[0] = 1 - p.sum()
    return place_one_each(rng, cap_diamonds(rng.choice(7, size=(h, w), p=p).astype(np.uint8)))


def platforms(rng, h, w, spikes=0.1, diamonds=0.1):
    """a floor, short platforms above it, the three objects standing on something, a few spikes and diamonds on the ground"""
    m = np.zeros((h, w), np.uint8)
    m[h - 1] = SOLID if h > 1 else EMPTY
    for y in range(h - 3, 0, -2):
        for _ in range(max(1, w // 5)):
            x0 = int(rng.integers(0, w))
            m[y, x0:x0 + int(rng.integers(2, 5))] = SOLID
    standing = [y * w + x for y in range(h - 1) for x in range(w) if m[y, x] == EMPTY and m[y + 1, x] == SOLID]
    if len(standing) < 3:
        standing = list(np.flatnonzero(m.ravel() == EMPTY))
    place_one_each(rng, m, standing)
    for at in standing:
        if m.ravel()[at] == EMPTY:
            u = rng.random()
            m.ravel()[at] = SPIKE if u < spikes else (DIAMOND if u < spikes + diamonds else EMPTY)
    return cap_diamonds(m)


def diamond_heavy(rng, h, w, share=0.5):
    """diamonds on a large share of the cells (at most 64), no spikes, little solid"""
    m = rng.choice(7, size=(h, w), p=[1 - share - 0.1, 0.1, 0, 0, share, 0, 0]).astype(np.uint8)
    return place_one_each(rng, cap_diamonds(m))


def spike_corridor(rng, h, w, gap=2):
    """one corridor above a floor with spikes standing in it every `gap` + 1 cells: the player at one end, the key in the
    middle, the exit at the other end; everything else solid"""
    m = np.full((h, w), SOLID, np.uint8)
    if h < 3 or w < 3:
        return place_one_each(rng, np.zeros((h, w), np.uint8))
    y = h - 2
    m[max(0, y - 2):y + 1, :] = EMPTY
    for x in range(2, w - 1, gap + 1):
        m[y, x] = SPIKE
    m[y, 0], m[y, w - 1] = PLAYER, EXIT
    mid = w // 2
    m[y, mid if m[y, mid] == EMPTY else mid - 1] = KEY
    if rng.random() < 0.5:
        m[y, :] = m[y, ::-1].copy()
    return m


def tall_shaft(rng, h, w):
    """solid but for one or two columns: the player falls or cannot climb"""
    m = np.full((h, w), SOLID, np.uint8)
    x = int(rng.integers(0, w))
    m[:, x] = EMPTY
    if w > 1 and rng.random() < 0.5:
        m[:, min(w - 1, x + 1)] = EMPTY
    free = np.flatnonzero(m.ravel() == EMPTY)
    place_one_each(rng, m, free)
    for at in free:
        if m.ravel()[at] == EMPTY and rng.random() < 0.15:
            m.ravel()[at] = DIAMOND
    return cap_diamonds(m)


GENERATORS = (random_level, chance_level, platforms, diamond_heavy, spike_corridor, tall_shaft)


def mixed(rng, h, w, n):
    """n maps, the generators in turn"""
    return np.stack([GENERATORS[i % len(GENERATORS)](rng, h, w) for i in range(n)])
