"""MiniDungeon maps for the fixtures (tools/gen_golden_mdungeon.py) and the GPU tests: uint8 [H][W] of tile ids 0..7 (empty,
solid, player, exit, potion, treasure, goblin, ogre).  Every generator works at any shape from 1 x 1 and never leaves more than
64 items (potions, treasures, enemies) on a map (the device's limit), so no generated level is left unsearched for that
reason."""
import numpy as np

EMPTY, SOLID, PLAYER, EXIT, POTION, TREASURE, GOBLIN, OGRE = range(8)
PROB = (0.4, 0.4, 0.02, 0.02, 0.03, 0.03, 0.05, 0.05)  # probs/mdungeon/mdungeon_prob.py:20 _prob, in tile order
MAX_ITEMS = 64


def cap_items(m):
    """the items past the 64th in row-major order become empty"""
    at = np.flatnonzero(m.ravel() >= POTION)
    m.ravel()[at[MAX_ITEMS:]] = EMPTY
    return m


def place_one_each(rng, m, where=None):
    """exactly one player and one exit, on distinct cells among `where` (flat indices; all cells by default): as many of the
    two as fit"""
    m[(m == PLAYER) | (m == EXIT)] = EMPTY
    cells = np.arange(m.size) if where is None else np.asarray(where)
    pick = rng.permutation(cells)[:2]
    for tile, at in zip((PLAYER, EXIT), pick):
        m.ravel()[at] = tile
    return m


def chance_level(rng, h, w, prob=PROB):
    """every cell from the tile probabilities: how many players and exits there are is left to chance"""
    return cap_items(rng.choice(8, size=(h, w), p=prob).astype(np.uint8))


def random_level(rng, h, w, solid=0.1, potion=0.03, treasure=0.06, goblin=0.08, ogre=0.08):
    """the other tiles from their probabilities, then one player and one exit"""
    p = np.array([0, solid, 0, 0, potion, treasure, goblin, ogre], float)
    p[0] = 1 - p.sum()
    return cap_items(place_one_each(rng, rng.choice(8, size=(h, w), p=p).astype(np.uint8)))


def sparse_level(rng, h, w):
    """few walls and few items: most of these reach the solver and win early"""
    return random_level(rng, h, w, solid=0.05, potion=0.02, treasure=0.02, goblin=0.03, ogre=0.02)


def rooms(rng, h, w):
    """walls every third row with one door each, items in the rooms, the player at the top and the exit at the bottom"""
    m = np.zeros((h, w), np.uint8)
    for y in range(2, h - 1, 3):
        m[y] = SOLID
        m[y, int(rng.integers(0, w))] = EMPTY
    free = np.flatnonzero(m.ravel() == EMPTY)
    for at in free:
        u = rng.random()
        m.ravel()[at] = (POTION if u < 0.04 else TREASURE if u < 0.10 else GOBLIN if u < 0.16 else OGRE if u < 0.20 else EMPTY)
    if len(free) >= 2:
        m.ravel()[free[0]], m.ravel()[free[-1]] = PLAYER, EXIT
        return cap_items(m)
    return place_one_each(rng, m)


def treasure_heavy(rng, h, w, share=0.3):
    """treasures on a large share of the cells (at most 64 items), a few enemies, little solid: every treasure is worth four
    steps to the A* stages, which wander"""
    m = rng.choice(8, size=(h, w), p=[1 - share - 0.15, 0.05, 0, 0, 0.02, share, 0.04, 0.04]).astype(np.uint8)
    return cap_items(place_one_each(rng, m))


def ogre_corridor(rng, h, w, ogres=3):
    """one corridor, everything else solid: the player at one end, the exit at the other, `ogres` ogres between them (three
    kill the player before the door), sometimes a potion or a goblin among them"""
    m = np.full((h, w), SOLID, np.uint8)
    if w < 3:
        return place_one_each(rng, np.zeros((h, w), np.uint8))
    y = h // 2
    m[y, :] = EMPTY
    m[y, 0], m[y, w - 1] = PLAYER, EXIT
    inner = list(range(1, w - 1))
    for i, x in enumerate(inner[:ogres]):
        m[y, x] = OGRE
    for x in inner[ogres:]:
        u = rng.random()
        m[y, x] = POTION if u < 0.15 else GOBLIN if u < 0.3 else EMPTY
    if rng.random() < 0.5:
        m[y, :] = m[y, ::-1].copy()
    return cap_items(m)


def gauntlet(rng, h, w):
    """an open map whose items are potions and enemies alone, dense: health goes up and down on every route"""
    m = rng.choice(8, size=(h, w), p=[0.45, 0.05, 0, 0, 0.15, 0, 0.2, 0.15]).astype(np.uint8)
    return cap_items(place_one_each(rng, m))


def guarded_exit(rng, h, w):
    """an open map with treasures and potions, the exit in a corner behind three diagonals of ogres: every route to the door
    costs six health, so no stage wins and each spends its budget on (position, health, items) states"""
    if h < 4 or w < 4:
        return random_level(rng, h, w)
    m = rng.choice(8, size=(h, w), p=[0.7, 0, 0, 0, 0.08, 0.17, 0.05, 0]).astype(np.uint8)
    for y in range(min(h, 5)):
        for x in range(min(w, 5)):
            m[y, x] = EXIT if x + y == 0 else OGRE if x + y <= 3 else EMPTY if x + y == 4 else m[y, x]
    m[h - 1, w - 1] = PLAYER
    if rng.random() < 0.5:
        m = m[::-1].copy()
    if rng.random() < 0.5:
        m = m[:, ::-1].copy()
    return cap_items(m)


GENERATORS = (random_level, chance_level, sparse_level, rooms, treasure_heavy, ogre_corridor, gauntlet, guarded_exit)


def mixed(rng, h, w, n):
    """n maps, the generators in turn"""
    return np.stack([GENERATORS[i % len(GENERATORS)](rng, h, w) for i in range(n)])
