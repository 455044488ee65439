"""The Lode Runner problem's rules in plain Python: what LoderunnerProblem.get_stats computes and the loss
ControlWrapper.get_loss would derive from it (file:line references are relative to the reference's
control_pcgrl/envs/probs/).  Test infrastructure: the fixtures under tests/golden/loderunner pin these rules to the
reference with its clock stopped, and the GPU tests pin the kernel to these rules.  The loss is a restatement only: the
reference cannot construct this problem any more, so ControlWrapper.get_loss cannot be run on it.

A map is an (H, W) array of tile ids (loderunner_prob.py:46); an id above 7 reads as empty.
"""
import heapq
import math

import numpy as np

TILES = ["empty", "brick", "ladder", "rope", "solid", "gold", "enemy", "player"]
CHARS = ".b#-BGEM"
STAT_KEYS = ["player", "enemies", "gold", "win", "path-length"]
EMPTY, BRICK, LADDER, ROPE, SOLID, GOLD, ENEMY, PLAYER = range(8)
LEFT, RIGHT, UP, DOWN, DLEFT, DRIGHT = range(6)
MOVE_NAMES = ["left", "right", "up", "down", "d-left", "d-right"]
DELTA = ((0, -1), (0, 1), (-1, 0), (1, 0), (1, -1), (1, 1))  # (row, column)
BLOCK = (BRICK, SOLID)            # what a "not b / B" test refuses
SUPPORT = (BRICK, SOLID, LADDER)  # what stops a fall and carries a step
FREE = (GOLD, ENEMY, EMPTY)       # what a sideways step or a diagonal fall may enter
HANG = (LADDER, ROPE)             # what a sideways step may grab
# frozen at the stock 12 x 8 whatever the map (loderunner_prob.py:13-14, loderunner_ctrl_prob.py:20)
MAX_PATH_LENGTH = float((math.ceil(12 / 2) * 8 + math.floor(8 / 2)) * 2 - 1)
STATIC_TRGS = {"player": 1, "enemies": 2, "gold": (1, 10), "win": 1, "path-length": MAX_PATH_LENGTH}
COND_BOUNDS = {"player": (0, 96), "enemies": (0, 96), "gold": (0, 10), "win": (0, 1), "path-length": (0, MAX_PATH_LENGTH)}
DEFAULT_WEIGHTS = {"player": 1, "enemies": 0, "gold": 0, "win": 1, "path-length": 0}  # loderunner_prob.py:35-44
NOT_COLLECTED, BY_OWN_SEARCHES, ON_ANOTHER_PATH, ON_THE_FALL = 0, 1, 2, 3


def clean(m):
    m = np.array(m, dtype=np.int64)
    m[(m < 0) | (m > 7)] = EMPTY
    return m


def moves(m, r, c):
    """Node.get_actions (loderunner/engine.py:52-165): the moves out of (r, c) in the order the engine lists them."""
    H, W = m.shape
    t = m[r, c]
    out = []
    bottom = r == H - 1

    def side(dc, name):  # the bottom row: anything but brick and solid is entered
        if 0 <= c + dc < W and m[r, c + dc] not in BLOCK:
            out.append(name)

    def walk(dc, name):  # above the bottom row: grab a ladder or a rope, or step onto a free cell that has support
        if 0 <= c + dc < W and (m[r, c + dc] in HANG or (m[r, c + dc] in FREE and m[r + 1, c + dc] in SUPPORT)):
            out.append(name)

    def drop(dc, name):  # a free cell without support: the step ends one row lower
        if 0 <= c + dc < W and m[r, c + dc] in FREE and m[r + 1, c + dc] not in SUPPORT:
            out.append(name)

    if t == LADDER:
        if bottom:
            side(-1, LEFT), side(1, RIGHT)
            if r != 0 and m[r - 1, c] not in BLOCK:
                out.append(UP)
        else:
            if r != 0 and m[r - 1, c] not in BLOCK:
                out.append(UP)
            if m[r + 1, c] not in BLOCK:
                out.append(DOWN)
            walk(-1, LEFT), walk(1, RIGHT), drop(-1, DLEFT), drop(1, DRIGHT)
    elif t == ROPE:
        if bottom:
            side(-1, LEFT), side(1, RIGHT)
        else:
            if m[r + 1, c] not in BLOCK:
                out.append(DOWN)
            walk(-1, LEFT), walk(1, RIGHT), drop(-1, DLEFT), drop(1, DRIGHT)
    elif t in FREE:
        if bottom:
            side(-1, LEFT), side(1, RIGHT)
        elif m[r + 1, c] not in SUPPORT:
            out.append(DOWN)  # falling: nothing else
        else:
            walk(-1, LEFT), walk(1, RIGHT)
            if m[r + 1, c] == LADDER:
                out.append(DOWN)
            drop(-1, DLEFT), drop(1, DRIGHT)
    # brick, solid and the left-behind player: no moves
    return out


def astar(m, src, goal, count=None, pushed=None):
    """AStar.run (engine.py:244-269) with the clock stopped: the cells from the goal back to the source and the moves taken
    in the same order, or None.  Ordered by (Manhattan distance + steps, insertion counter); the goal test is made on pop.
    `count[0]` counts the cells expanded; `pushed` (a set) receives every child cell."""
    cnt = 0
    heap = [(abs(src[0] - goal[0]) + abs(src[1] - goal[1]), 0, src, None, 0, None)]
    closed = {}
    while heap:
        _, _, cell, parent, step, move = heapq.heappop(heap)
        if cell in closed:
            continue
        if cell == goal:
            cells, taken = [cell], []
            while parent is not None:
                cells.append(parent)
                taken.append(move)
                parent, move = closed[parent]
            return cells, taken
        closed[cell] = (parent, move)
        if count is not None:
            count[0] += 1
        for mv in moves(m, *cell):
            child = (cell[0] + DELTA[mv][0], cell[1] + DELTA[mv][1])
            cnt += 1
            if pushed is not None:
                pushed.add(child)
            heapq.heappush(heap, (abs(child[0] - goal[0]) + abs(child[1] - goal[1]) + step + 1, cnt, child, cell, step + 1, mv))
    return None


def start(m):
    """get_starting_point (engine.py:323-338) for a map with one player: landing row, column, golds collected on the way."""
    H, W = m.shape
    r, c = [int(v) for v in np.argwhere(m == PLAYER)[0]]
    fallen = []
    while r != H - 1 and m[r + 1, c] not in SUPPORT and m[r, c] != ROPE:
        r += 1
        if m[r, c] == GOLD:
            fallen.append((r, c))
    return r, c, fallen


def play(m, record=None, pushed=None):
    """get_score (engine.py:368-389) with the clock stopped.  Returns a dict: win, path_length, landing, collected, golds (all,
    row-major), state and dist per gold, expanded (cells expanded over all searches), longest (by one search).  `record`: a list that receives
    (gold, to_goal, to_start) with the astar results of every pair of searches that ran."""
    m = clean(m)
    golds = [(int(r), int(c)) for r, c in np.argwhere(m == GOLD)]
    r, c, fallen = start(m)
    m[r, c] = EMPTY
    state = {g: (ON_THE_FALL if g in fallen else NOT_COLLECTED) for g in golds}
    dist = {g: 0 for g in golds}
    out = {"landing": (r, c), "golds": golds, "expanded": 0}
    count = [0]
    total = longest = 0
    if not golds:
        win = -1
    else:
        for g in golds:
            if state[g] != NOT_COLLECTED:
                continue
            before = count[0]
            to_goal = astar(m, (r, c), g, count, pushed)
            middle = count[0]
            to_start = astar(m, g, (r, c), count, pushed) if to_goal is not None else None
            longest = max(longest, middle - before, count[0] - middle)
            if record is not None:
                record.append((g, to_goal, to_start))
            if to_start is None:
                continue
            state[g] = BY_OWN_SEARCHES
            dist[g] = len(to_goal[0])
            total += dist[g]
            for cells, _ in (to_goal, to_start):
                for p in cells[1:]:  # the parents: the path's destination is not looked at
                    if m[p] == GOLD and state.get(p) == NOT_COLLECTED:
                        state[p] = ON_ANOTHER_PATH
        collected = sum(1 for g in golds if state[g] != NOT_COLLECTED)
        win = 1 / (1 + (len(golds) - collected))
    out.update(win=win, path_length=total, collected=sum(1 for g in golds if state[g] != NOT_COLLECTED),
               state=[state[g] for g in golds], dist=[dist[g] for g in golds], expanded=count[0], longest=longest)
    return out


def get_stats(m):
    """LoderunnerProblem.get_stats (loderunner_prob.py:78-91): (the five statistics in order, the play record or None)."""
    m = clean(m)
    stats = [int((m == PLAYER).sum()), int((m == ENEMY).sum()), int((m == GOLD).sum()), 0, 0]
    rec = None
    if stats[0] == 1:
        rec = play(m)
        stats[3], stats[4] = rec["win"], rec["path_length"]
    return stats, rec


def outputs(m, gold_cap=32):
    """What the device reports for one map: stats (5 floats), play (4 ints), gold_state and gold_dist ([gold_cap])."""
    stats, rec = get_stats(m)
    gs, gd = [-1] * gold_cap, [0] * gold_cap
    if rec is None:
        golds = int(stats[2])
        for j in range(min(golds, gold_cap)):
            gs[j] = 0
        return [float(s) for s in stats], [0, -1, -1, 0], gs, gd
    for j in range(min(len(rec["golds"]), gold_cap)):
        gs[j], gd[j] = rec["state"][j], rec["dist"][j]
    return [float(s) for s in stats], [1, rec["landing"][0], rec["landing"][1], rec["collected"]], gs, gd


def target_interval(trg):
    """control_wrappers.py:334-341: a tuple target (lo, hi) is arange(lo, hi), the upper end excluded."""
    if isinstance(trg, tuple):
        return float(trg[0]), float(trg[1] - 1)
    return float(trg), float(trg)


def loss(stats, weights=None, trgs=None):
    """ControlWrapper.get_loss (control_wrappers.py:318-345) restated: over the statistics in order,
    loss += -(distance of the value to its target interval) * weight."""
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
