"""The Super Mario Bros problem's rules in plain integers: what SMBCtrlProblem.get_stats and ControlWrapper.get_loss compute
(file:line references are relative to the reference's control_pcgrl/).  Test infrastructure: the
fixtures under tests/golden/smb pin these rules to the reference, and the GPU tests pin the kernel to these rules.

A map is an (H, W) array of tile ids: 0 empty, 1 solid, 2 enemy, 3 brick, 4 question, 5 coin, 6 tube (smb_prob.py:12).
"""
import heapq

import numpy as np

STAT_KEYS = ["dist-floor", "disjoint-tubes", "enemies", "empty", "noise", "jumps", "jumps-dist", "dist-win", "sol-length"]
EMPTY, SOLID, ENEMY, BRICK, QUESTION, COIN, TUBE = range(7)
FLOOR = (SOLID, BRICK, QUESTION)       # get_stats lists tube_left / tube_right too, which never occur in a map
BLOCKING = (SOLID, BRICK, QUESTION, TUBE)  # gameCharacters " # ## #" (smb_prob.py:97)
ACTIONS = ((0, 0), (1, 0), (0, -1), (1, -1))  # engine.py:3
# frozen at the stock 16 x 116 whatever the map (smb_prob.py:16-26, smb_ctrl_prob.py:8-36)
STATIC_TRGS = {"dist-floor": 0, "disjoint-tubes": 0, "enemies": (10, 30), "empty": (900, 1856), "noise": 0,
               "jumps": (20, 1856), "jumps-dist": 0, "dist-win": 0, "sol-length": 348}
DEFAULT_WEIGHTS = {"dist-floor": 2, "disjoint-tubes": 1, "enemies": 1, "empty": 1, "noise": 4, "jumps": 2, "jumps-dist": 2,
                   "dist-win": 5, "sol-length": 1}  # configs/config.py SMBConfig


def map_stats(m):
    """dist-floor, disjoint-tubes, enemies, empty, noise (helper.py:40-140)."""
    m = np.asarray(m)
    H, W = m.shape
    dist_floor = 0
    for y in range(H):
        for x in range(W):
            if m[y, x] != ENEMY:
                continue
            d = H - 1
            for dy in range(1, H - y):
                if m[y + dy, x] in FLOOR:
                    d = dy - 1
                    break
            dist_floor += d
    tubes = 0
    for y in range(H):
        for x in range(W):
            if m[y, x] == TUBE:
                nb = int(x > 0 and m[y, x - 1] == TUBE) + int(x < W - 1 and m[y, x + 1] == TUBE)
                tubes += nb == 1
    noise = int((m[:, 1:] != m[:, :-1]).sum()) + int((m[1:, :] != m[:-1, :]).sum())
    return [int(dist_floor), int(tubes), int((m == ENEMY).sum()), int((m == EMPTY).sum()), noise]


def build_level(m):
    """(solid[H][W + 6], exit column, start x, start y): smb_prob.py:96-119, engine.py:137-178."""
    m = np.asarray(m)
    H, W = m.shape
    assert H >= 4, "with fewer than 4 rows the level has no exit row"
    solid = np.zeros((H, W + 6), dtype=bool)
    solid[:, 3:W + 3] = np.isin(m, BLOCKING)
    solid[H - 2:, :3] = True
    solid[H - 2:, W + 3:] = True
    solid[H - 3, W + 4] = True
    return solid, W + 4, 1, H - 3


def _movable(solid, x, y):
    if y < 0:
        return True
    H, LW = solid.shape
    return not (x < 0 or x >= LW or y >= H or solid[y][x])


def move(solid, x, y, air, a):
    """State.update (engine.py:197-237) -> (x, y, airTime, jumped)."""
    H = solid.shape[0]
    dx, dy = ACTIONS[a]
    ground = bool(solid[y + 1][x]) if -1 <= y < H - 1 else False
    nx, ny, jumped = x, y, False
    if dx and _movable(solid, nx + 1, ny):
        nx += 1
    if dy == -1:
        if ground and _movable(solid, nx, ny - 1):
            air, jumped = 5, True
    elif air > 0:
        air = 1
    if air > 1:
        air -= 1
        if _movable(solid, nx, ny - 1):
            ny -= 1
        else:
            air = 1
    elif air == 1:
        air = 0
    elif _movable(solid, nx, ny + 1):
        ny += 1
    assert -5 <= ny <= H
    return nx, ny, air, jumped


class _Entry:
    """What the heap orders: f alone, as Node.__lt__ (engine.py:54) -- ties are left to heapq's sift order."""
    __slots__ = ("f", "node")

    def __init__(self, f, node):
        self.f, self.node = f, node

    def __lt__(self, other):
        return self.f < other.f


def search(solid, ex, sx, sy, balance, power):
    """AStarAgent.getSolution (engine.py:105-129).  A node is (x, y, air, jumps, depth, parent, action, jump_loc)."""
    H = solid.shape[0]
    nodes = [(sx, sy, 0, 0, 0, -1, -1, None)]
    heap = [_Entry(ex - sx, 0)]
    seen, best, iterations = set(), -1, 0
    while iterations < power and heap:
        iterations += 1
        cur = heapq.heappop(heap).node
        x, y, air, jumps, depth = nodes[cur][:5]
        if y >= H:
            continue
        if x >= ex:
            return cur, nodes, iterations
        if (x, y, air) in seen:
            continue
        if best < 0 or ex - x < ex - nodes[best][0] or (x == nodes[best][0] and depth < nodes[best][4]):
            best = cur
        seen.add((x, y, air))
        for a in range(4):
            nx, ny, nair, jumped = move(solid, x, y, air, a)
            nodes.append((nx, ny, nair, jumps + jumped, depth + 1, cur, a, (x, y) if jumped else None))
            heapq.heappush(heap, _Entry((ex - nx) + balance * (depth + 1), len(nodes) - 1))
    return best, nodes, iterations


def trace(nodes, i):
    """(moves, jump locations) of node i, root first."""
    moves, locs = [], []
    while nodes[i][5] >= 0:
        moves.append(nodes[i][6])
        if nodes[i][7] is not None:
            locs.append(nodes[i][7])
        i = nodes[i][5]
    return moves[::-1], locs[::-1]


def run_pass(m, balance, power):
    """One getSolution call on the level of map m, as a dict of plain values."""
    solid, ex, sx, sy = build_level(m)
    i, nodes, iterations = search(solid, ex, sx, sy, balance, power)
    moves, locs = trace(nodes, i)
    x, y, air, jumps = nodes[i][:4]
    return {"moves": moves, "jump_locs": locs, "won": int(x >= ex), "x": x, "y": y, "air": air, "jumps": jumps,
            "iterations": iterations, "ex": ex}


def play(m, power):
    """SMBProblem._run_game: balance 1, then balance 0 when the first did not win; the result is the last pass run."""
    p1 = run_pass(m, 1, power)
    if p1["won"]:
        return p1, p1["iterations"], 0
    p2 = run_pass(m, 0, power)
    return p2, p1["iterations"], p2["iterations"]


def get_stats(m, power=10000):
    """The nine statistics in STAT_KEYS order, and the play-through record."""
    m = np.asarray(m)
    W = m.shape[1]
    res, it1, it2 = play(m, power)
    value, prev = 0, 0
    for (jx, _) in res["jump_locs"]:  # jx is a level x (offset 3); W is the map's width: kept as the reference has it
        value = max(value, jx - prev)
        prev = jx
    value = max(value, W - prev)
    stats = map_stats(m) + [res["jumps"], value, 0 if res["won"] else res["ex"] - res["x"],
                            len(res["moves"]) if res["won"] else 0]
    rec = dict(res, it1=it1, it2=it2)
    return stats, rec


def target_distance(trg, val):
    if isinstance(trg, tuple):  # min |arange(lo, hi) - val|: the upper end is excluded (control_wrappers.py:339)
        lo, hi = trg[0], trg[1] - 1
        return lo - val if val < lo else (val - hi if val > hi else 0)
    return abs(trg - val)


def loss(stats, weights=None):
    """ControlWrapper.get_loss (control_wrappers.py:318-345)."""
    weights = DEFAULT_WEIGHTS if weights is None else weights
    total = 0.0
    for k, v in zip(STAT_KEYS, stats):
        total += -float(target_distance(STATIC_TRGS[k], v)) * float(weights[k])
    return total
