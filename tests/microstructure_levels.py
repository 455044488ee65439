"""Microstructure maps for the fixtures and the GPU tests (0 empty, 1 solid): random two-phase maps, the extremes, and hand-made
maps with an exact number of regions.  Test infrastructure; nothing here comes from the reference."""
import numpy as np

EMPTY, SOLID = 0, 1


def random_map(rng, h, w, p_empty=None):
    """each cell empty with probability p_empty (drawn from 0.4 .. 0.7 if not given)"""
    p = rng.uniform(0.4, 0.7) if p_empty is None else p_empty
    return (rng.random((h, w)) >= p).astype(np.uint8)


def all_solid(h, w):
    return np.ones((h, w), np.uint8)


def all_empty(h, w):
    return np.zeros((h, w), np.uint8)


def one_cell(h, w, r, c):
    m = all_solid(h, w)
    m[r, c] = EMPTY
    return m


def checkerboard(h, w, first_empty=True):
    """every empty cell a region of its own: ceil(h * w / 2) regions when the first cell is empty"""
    rr, cc = np.indices((h, w))
    return (((rr + cc) % 2 == 0) != first_empty).astype(np.uint8)


def serpentine(h, w):
    """one corridor through every even row, joined at alternating ends: the longest shortest path a map of this size has"""
    m = all_solid(h, w)
    m[0::2, :] = EMPTY
    for k, r in enumerate(range(1, h - 1, 2)):
        m[r, w - 1 if k % 2 == 0 else 0] = EMPTY
    return m


def cross(h, w, arm):
    """a plus-shaped region in the top-left corner: from the tip of its upper arm the three other tips are equally far"""
    m = all_solid(h, w)
    m[arm, 0:2 * arm + 1] = EMPTY
    m[0:2 * arm + 1, arm] = EMPTY
    return m


def equal_pair(h, w):
    """two regions with the same d: a row segment and a column segment of the same length"""
    m = all_solid(h, w)
    k = min(h, w) // 2
    m[0, 0:k] = EMPTY
    m[h - k:h, w - 1] = EMPTY
    return m


BLOCK_H, BLOCK_W = 4, 5  # an L of up to 3 x 4 cells and its solid margin


def l_shapes(rng, h, w, count):
    """exactly `count` regions, one per 4 x 5 block in row-major block order: L-shaped regions with arms of 0..2 rows and 0..3
    columns in one of four orientations (a = b = 0 is a one-cell region), so the regions' values differ"""
    nby, nbx = h // BLOCK_H, w // BLOCK_W
    assert count <= nby * nbx, (h, w, count)
    m = all_solid(h, w)
    forms = [(a, b, fr, fc) for a in range(3) for b in range(4) for fr in range(2) for fc in range(2)]
    order = rng.permutation(len(forms))  # every form once before any comes again
    for k in range(count):
        r0, c0 = (k // nbx) * BLOCK_H, (k % nbx) * BLOCK_W
        a, b, fr, fc = forms[order[k % len(forms)]]
        corner_r = r0 + (a if fr else 0)
        corner_c = c0 + (b if fc else 0)
        m[r0:r0 + a + 1, corner_c] = EMPTY
        m[corner_r, c0:c0 + b + 1] = EMPTY
    return m


def batch(seed, n, h, w):
    """n random maps, empty share drawn per map from 0.4 .. 0.7"""
    rng = np.random.default_rng(seed)
    return np.stack([random_map(rng, h, w) for _ in range(n)])
