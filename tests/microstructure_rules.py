"""The microstructure problem's rules in plain Python / numpy: what MicroStructureProblem.get_stats computes
(microstructure/microstructure_prob.py:107-119 -> helper.py:278-318 calc_tortuosity, :225-240 run_dijkstra) and the loss
ControlWrapper.get_loss would derive from it (file:line references are relative to the reference's
control_pcgrl/envs/).  Test infrastructure: the fixtures under tests/golden/microstructure pin these rules to the reference,
and the GPU tests pin the kernel to these rules.  The loss is a restatement only: the reference cannot construct this problem
any more, so ControlWrapper.get_loss cannot be run on it.

A map is an (H, W) array of tile ids, 0 empty and 1 solid; any other id reads as solid.
"""
import math
from collections import deque

import numpy as np

TILES = ["empty", "solid"]
STAT_KEYS = ["path-length", "tortuosity"]
EMPTY, SOLID = 0, 1
# frozen at the stock 64 x 64 whatever the map (microstructure_prob.py:17-18, :32-51)
MAX_PATH_LENGTH = float(math.ceil(64 / 2) * 64 + math.floor(64 / 2))  # 2080.0
MAX_TORTUOSITY = MAX_PATH_LENGTH / 2  # 1040.0
STATIC_TRGS = {"tortuosity": MAX_TORTUOSITY}
COND_BOUNDS = {"path-length": (0, MAX_PATH_LENGTH), "tortuosity": (0, MAX_TORTUOSITY)}
DEFAULT_WEIGHTS = {"tortuosity": 1}  # microstructure_prob.py:24-29 _reward_weights
REC_FIELDS = 5  # start row, start column, far row, far column, d


def clean(m):
    m = np.array(m, dtype=np.int64)
    m[m != EMPTY] = SOLID
    return m


def flood(passable, r, c):
    """run_dijkstra (helper.py:225-240): a first-in first-out flood, so the map holds breadth-first distances; -1 where the
    flood did not come."""
    H, W = passable.shape
    dist = np.full((H, W), -1, dtype=np.int64)
    if not passable[r, c]:
        return dist
    dist[r, c] = 0
    todo = deque([(r, c)])
    while todo:
        y, x = todo.popleft()
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and passable[ny, nx] and dist[ny, nx] < 0:
                dist[ny, nx] = dist[y, x] + 1
                todo.append((ny, nx))
    return dist


def regions(m):
    """The loop of calc_tortuosity (helper.py:292-309): one entry per region in visit order -- the row-major order of the
    regions' first cells -- as (start row, start column, far row, far column, d, tort)."""
    passable = clean(m) == EMPTY
    H, W = passable.shape
    visited = np.zeros((H, W), dtype=bool)
    out = []
    for y in range(H):  # get_tile_locations (helper.py:19-26): rows outer, columns inner
        for x in range(W):
            if not passable[y, x] or visited[y, x]:
                continue
            dist = flood(passable, y, x)
            visited |= dist >= 0
            my, mx = np.unravel_index(np.argmax(dist, axis=None), dist.shape)  # the FIRST cell at the greatest distance
            d = int(np.max(flood(passable, int(my), int(mx))))
            l2 = np.sqrt((x - int(mx)) ** 2 + (y - int(my)) ** 2)
            l2 = l2 if l2 > 0 else 1
            out.append((y, x, int(my), int(mx), d, float(np.float64(d) / np.float64(l2))))
    return out


def numpy_sum(v):
    """What numpy's add.reduce gives for a contiguous float64 vector: the pairwise sum of
    numpy/core/src/umath/loops_utils.h.src, written out.  tests/test_microstructure_cpu.py checks it against np.mean bit for
    bit for every length 0 .. 2 100."""
    v = [float(x) for x in v]
    n = len(v)
    if n < 8:
        res = 0.0
        for x in v:
            res = res + x
        return res
    if n <= 128:
        r = v[:8]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = r[j] + v[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res = res + v[i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return numpy_sum(v[:n2]) + numpy_sum(v[n2:])


def numpy_mean(v):
    """np.mean of a non-empty float64 vector: the sum above, then one division by the count"""
    return numpy_sum(v) / float(len(v))


def get_stats(m):
    """[path-length, tortuosity] as floats (the reference returns the integer 0 for both when there is no empty cell)"""
    regs = regions(m)
    path = 0
    for r in regs:
        if r[4] > path:  # replaced only on `>` (helper.py:301)
            path = r[4]
    tort = numpy_mean([r[5] for r in regs]) if regs else 0.0
    return [float(path), float(tort)]


def outputs(m, cap):
    """What pcgrl_microstructure_evaluate writes for one map: stats, the region count, and with cap > 0 region_rec [cap][5]
    (all -1 past the last region) and region_tort [cap] (0 past it)."""
    regs = regions(m)
    rec = [[-1] * REC_FIELDS for _ in range(cap)]
    tort = [0.0] * cap
    for i, r in enumerate(regs[:cap]):
        rec[i] = list(r[:5])
        tort[i] = r[5]
    return get_stats(m), len(regs), rec, tort


def has_error(m):
    m = np.asarray(m)
    return bool(((m != EMPTY) & (m != SOLID)).any())


def target_interval(trg):
    """control_wrappers.py:334-341: a tuple target (lo, hi) is arange(lo, hi), the upper end excluded."""
    if isinstance(trg, tuple):
        return float(trg[0]), float(trg[1] - 1)
    return float(trg), float(trg)


def loss(stats, weights=None, trgs=None):
    """ControlWrapper.get_loss (control_wrappers.py:318-345) restated: over the statistics in order,
    loss += -(distance of the value to its target interval) * weight.  path-length has no target and adds nothing."""
    weights = DEFAULT_WEIGHTS if weights is None else weights
    trgs = STATIC_TRGS if trgs is None else trgs
    total = 0.0
    for k, v in zip(STAT_KEYS, stats):
        if k not in trgs:
            continue
        lo, hi = target_interval(trgs[k])
        v = float(v)
        d = lo - v if v < lo else (v - hi if v > hi else 0.0)
        total = total + (-d * float(weights.get(k, 0.0)))
    return total
