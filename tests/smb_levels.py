"""A seeded generator of Super Mario Bros maps for the smb tests and tools: structured levels (floor, gaps, tubes,
platforms, enemies), uniform random levels with random tile probabilities, and walled-off levels nobody can finish.
Test infrastructure; tile ids as in tests/smb_rules.py."""
import numpy as np

EMPTY, SOLID, ENEMY, BRICK, QUESTION, COIN, TUBE = range(7)
KINDS = ("structured", "random", "walled")


def structured(rng, h, w, gap_prob=0.06, tube_prob=0.04, platform_prob=0.08, enemy_prob=0.05):
    m = np.zeros((h, w), dtype=np.uint8)
    floor = max(1, min(2, h - 2))  # rows of floor
    m[h - floor:, :] = SOLID
    x = int(rng.integers(0, 4))
    while x < w:
        r = rng.random()
        if r < gap_prob:  # a gap in the floor, 1..4 wide
            g = int(rng.integers(1, 5))
            m[h - floor:, x:x + g] = EMPTY
            x += g + 1
        elif r < gap_prob + tube_prob and h - floor >= 3:  # a tube 1..3 wide standing on the floor
            tw, th = int(rng.integers(1, 4)), int(rng.integers(1, min(5, h - floor - 1)))
            m[h - floor - th:h - floor, x:x + tw] = TUBE
            x += tw + 1
        elif r < gap_prob + tube_prob + platform_prob and h - floor >= 5:  # a platform of bricks and question blocks
            pw, py = int(rng.integers(2, 7)), h - floor - int(rng.integers(3, min(9, h - floor)))
            seg = m[py, x:x + pw]
            seg[:] = np.where(rng.random(seg.shape[0]) < 0.25, QUESTION, BRICK)
            if py > 0 and rng.random() < 0.5:
                m[py - 1, x:x + pw] = np.where(rng.random(seg.shape[0]) < 0.5, COIN, EMPTY)[:seg.shape[0]]
            x += pw + 1
        elif r < gap_prob + tube_prob + platform_prob + enemy_prob:  # an enemy on the ground, in the air or over a gap
            y = h - floor - 1 - (int(rng.integers(0, max(1, h - floor))) if rng.random() < 0.3 else 0)
            if m[y, x] == EMPTY:
                m[y, x] = ENEMY
            x += 1
        else:
            x += 1
    return m


def random_level(rng, h, w):
    p = rng.dirichlet(np.array([6.0, 1.0, 0.3, 0.6, 0.3, 0.4, 0.4]))
    return rng.choice(7, size=(h, w), p=p).astype(np.uint8)


def walled(rng, h, w):
    m = structured(rng, h, w, gap_prob=0.02)
    x = int(rng.integers(w // 2, w)) if w > 1 else 0
    m[:, x] = SOLID if rng.random() < 0.5 else TUBE  # a full-height wall: it can still be passed above row 0
    if rng.random() < 0.7:  # ... unless nothing near it is high enough to jump from
        m[:max(0, h - 2), max(0, x - 8):x] = EMPTY
    return m


def make(kind, seed, h, w):
    rng = np.random.default_rng([KINDS.index(kind), int(seed), h, w])
    return {"structured": structured, "random": random_level, "walled": walled}[kind](rng, h, w)


def batch(seed, n, h, w, kinds=KINDS):
    """n maps, cycling through `kinds`."""
    return np.stack([make(kinds[i % len(kinds)], seed * 100003 + i, h, w) for i in range(n)])
