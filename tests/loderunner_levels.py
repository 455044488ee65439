"""Lode Runner maps for the fixtures, the GPU tests and the benchmark (tests/loderunner_rules.py has the tile ids).  Every
generator is a pure function of its numpy Generator, so a seed names a set."""
import numpy as np

EMPTY, BRICK, LADDER, ROPE, SOLID, GOLD, ENEMY, PLAYER = range(8)
# LoderunnerProblem._prob (loderunner_prob.py:15) in tile-id order; it sums to 1.032 and is normalised here
PROB = np.array([0.56, 0.23, 0.10, 0.032, 0.03, 0.02, 0.05, 0.01])
KINDS = ("random", "gold", "structured")


def _one_player(rng, m):
    """exactly one player: the others become empty, or a random cell becomes the player"""
    m[m == PLAYER] = EMPTY
    m[rng.integers(m.shape[0]), rng.integers(m.shape[1])] = PLAYER
    return m


def random_level(rng, h, w, keep_players=False):
    """cells drawn from the problem's _prob; unless keep_players, exactly one of them is the player"""
    m = rng.choice(8, size=(h, w), p=PROB / PROB.sum()).astype(np.uint8)
    return m if keep_players else _one_player(rng, m)


def gold_level(rng, h, w):
    """a quarter of the cells gold, the rest mostly open: many searches, long other-gold chains"""
    p = np.array([0.38, 0.10, 0.12, 0.08, 0.02, 0.25, 0.05, 0.0])
    return _one_player(rng, rng.choice(8, size=(h, w), p=p / p.sum()).astype(np.uint8))


def structured_level(rng, h, w):
    """floors of brick every second or third row with gaps, ladders through them, ropes under some, golds on and off the
    platforms, a few enemies, one player somewhere in the air"""
    m = np.zeros((h, w), dtype=np.uint8)
    r = h - 1 - int(rng.integers(0, 2))
    while r >= 1:
        m[r, :] = BRICK if rng.random() < 0.8 else SOLID
        for _ in range(int(rng.integers(0, 3))):  # gaps
            c = int(rng.integers(w))
            m[r, c:c + int(rng.integers(1, 3))] = EMPTY
        for _ in range(int(rng.integers(1, 3))):  # ladders through the floor, up to the next one
            c = int(rng.integers(w))
            m[max(r - int(rng.integers(1, 4)), 0):r + 1, c] = LADDER
        if rng.random() < 0.5 and r + 1 < h:  # a rope under the floor
            c = int(rng.integers(w))
            m[r + 1, c:c + int(rng.integers(2, 5))] = ROPE
        r -= int(rng.integers(2, 4))
    free = np.argwhere(m == EMPTY)
    if len(free):
        for _ in range(int(rng.integers(1, max(2, h * w // 12)))):
            m[tuple(free[rng.integers(len(free))])] = GOLD
        for _ in range(int(rng.integers(0, 3))):
            m[tuple(free[rng.integers(len(free))])] = ENEMY
        m[tuple(free[rng.integers(len(free))])] = PLAYER
    else:
        _one_player(rng, m)
    return m


def level(kind, rng, h, w):
    return {"random": random_level, "gold": gold_level, "structured": structured_level}[kind](rng, h, w)


def batch(kind, seed, n, h, w):
    """n maps of one kind, uint8 [n][h][w]"""
    rng = np.random.default_rng(seed)
    return np.stack([level(kind, rng, h, w) for _ in range(n)])


def mixed(seed, n, h, w):
    """the three kinds in turn, and every eighth map with the player count left to chance (0, 1 or more)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 8 == 7:
            out.append(random_level(rng, h, w, keep_players=True))
        else:
            out.append(level(KINDS[i % 3], rng, h, w))
    return np.stack(out)
