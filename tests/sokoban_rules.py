"""Sokoban rules in plain Python, for the solution tests (test_solutions_cpu.py, test_gpu_solutions.py, tools/gen_golden_solutions.py).

Two things, both written from the rules and from nothing of the engine:

  replay(grid, moves)     plays a move list on a map: walls stop the player, a crate is pushed if the cell behind it is free
                          (one crate at a time), the level is won when every target carries a crate.
  solve(grid, power)      the reference's solver cascade (sokoban_prob.py:99-148 + sokoban/engine.py): BFSAgent, then AStarAgent
                          with balance 1, 0.5, 0, each limited to `power` iterations.  FIFO list; heapq whose entries compare by
                          h + balance * depth ONLY (Node.__lt__); visited set keyed on the player plus the ORDERED crate list;
                          the win test comes before the visited test; children in `directions` order, a child whose player did
                          not move is dropped, a push that leaves any crate on a dead cell is dropped (the deadlock table).

Tile ids: 0 empty, 1 solid, 2 player, 3 crate, 4 target.  Moves are indices into DIRECTIONS (the reference's `directions`,
engine.py:3).  Level coordinates are map coordinates + 1 (the one-tile solid border _run_game puts around the map).  Meant for
small rooms: a stage that runs to a cap of 10 000 iterations takes about a second.
"""
import heapq

import numpy as np

EMPTY, SOLID, PLAYER, CRATE, TARGET = range(5)
DIRECTIONS = ((-1, 0), (1, 0), (0, -1), (0, 1))  # (dx, dy)
AS_DICTS = tuple({"x": dx, "y": dy} for dx, dy in DIRECTIONS)


def precondition(grid):
    """one player, crates == targets > 0, one 4-connected region of non-solid cells (sokoban_prob.py:172-177)"""
    g = np.asarray(grid)
    if (g == PLAYER).sum() != 1 or (g == CRATE).sum() != (g == TARGET).sum() or (g == CRATE).sum() == 0:
        return False
    free = g != SOLID
    cells = np.argwhere(free)
    seen = np.zeros(g.shape, bool)
    stack = [tuple(cells[0])]
    seen[stack[0]] = True
    while stack:
        y, x = stack.pop()
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < g.shape[0] and 0 <= xx < g.shape[1] and free[yy, xx] and not seen[yy, xx]:
                seen[yy, xx] = True
                stack.append((yy, xx))
    return int(seen.sum()) == len(cells)


def replay(grid, moves):
    """-> (won, legal): the level after `moves` has a crate on every target; every move moved the player"""
    g = np.asarray(grid)
    h, w = g.shape
    solid = g == SOLID
    (py, px), = np.argwhere(g == PLAYER)
    crates = {(int(x), int(y)) for y, x in np.argwhere(g == CRATE)}
    targets = {(int(x), int(y)) for y, x in np.argwhere(g == TARGET)}
    px, py = int(px), int(py)
    legal = True

    def free(x, y):
        return 0 <= x < w and 0 <= y < h and not solid[y, x] and (x, y) not in crates

    for m in moves:
        dx, dy = DIRECTIONS[int(m)]
        nx, ny = px + dx, py + dy
        if free(nx, ny):
            px, py = nx, ny
        elif (nx, ny) in crates and free(nx + dx, ny + dy):
            crates.remove((nx, ny))
            crates.add((nx + dx, ny + dy))
            px, py = nx, ny
        else:
            legal = False
    return len(targets) > 0 and crates == targets, legal


class Level:
    """the bordered level of a map: solid[y][x], the player, crates and targets in row-major order, the dead cells"""

    def __init__(self, grid):
        g = np.asarray(grid)
        self.h, self.w = g.shape[0] + 2, g.shape[1] + 2
        b = np.full((self.h, self.w), SOLID, np.uint8)
        b[1:-1, 1:-1] = g
        self.solid = [[bool(v == SOLID) for v in row] for row in b]
        (y, x), = np.argwhere(b == PLAYER)
        self.player = (int(x), int(y))
        self.crates = tuple((int(x), int(y)) for y, x in np.argwhere(b == CRATE))
        self.targets = tuple((int(x), int(y)) for y, x in np.argwhere(b == TARGET))
        self.dead = self._dead_cells()

    def _dead_cells(self):
        """engine.py:203-246: a free non-target cell in a corner of walls is dead; so is every cell strictly between two such
        corners of one row (column) when every cell between them is free, no target and walled above or below (left or right)"""
        s, tg = self.solid, set(self.targets)
        corners = []
        for y in range(1, self.h - 1):
            for x in range(1, self.w - 1):
                if s[y][x] or (x, y) in tg:
                    continue
                if (s[y - 1][x] or s[y + 1][x]) and (s[y][x - 1] or s[y][x + 1]):
                    corners.append((x, y))
        dead = set(corners)
        for ax, ay in corners:
            for bx, by in corners:
                if ay == by and ax < bx:
                    run = [(x, ay) for x in range(ax + 1, bx)]
                    ok = all(not s[y][x] and (x, y) not in tg and (s[y - 1][x] or s[y + 1][x]) for x, y in run)
                elif ax == bx and ay < by:
                    run = [(ax, y) for y in range(ay + 1, by)]
                    ok = all(not s[y][x] and (x, y) not in tg and (s[y][x - 1] or s[y][x + 1]) for x, y in run)
                else:
                    continue
                if ok:
                    dead.update(run)
        return frozenset(dead)

    def heuristic(self, crates):
        """engine.py:282-296: crates in list order greedily take the nearest remaining target, the first of equals"""
        left = list(self.targets)
        total = 0
        for cx, cy in crates:
            best, at = self.w + self.h, 0
            for i, (tx, ty) in enumerate(left):
                d = abs(cx - tx) + abs(cy - ty)
                if best > d:
                    best, at = d, i
            tx, ty = left.pop(at)
            total += abs(tx - cx) + abs(ty - cy)
        return total


class _Entry:
    """an open-list entry: compares by its key only, as Node.__lt__ does"""
    __slots__ = ("key", "node")

    def __init__(self, key, node):
        self.key, self.node = key, node

    def __lt__(self, other):
        return self.key < other.key


def _stage(lv, balance2, power, directions):
    """one agent's getSolution: balance2 None = BFSAgent, else AStarAgent with balance = balance2 / 2.
    -> (won, moves of the returned node, its heuristic, the open list ran dry)"""
    target_set = set(lv.targets)
    # node records: parent, move, depth, h, player, crates
    h0 = lv.heuristic(lv.crates)
    nodes = [(-1, -1, 0, h0, lv.player, lv.crates)]
    fifo, head, heap = [0], 0, [_Entry(2 * h0, 0)]
    visited = set()
    best = None
    iters = 0

    def actions(n):
        out = []
        while nodes[n][0] >= 0:
            out.append(nodes[n][1])
            n = nodes[n][0]
        return out[::-1]

    while iters < power and (head < len(fifo) if balance2 is None else len(heap) > 0):
        iters += 1
        if balance2 is None:
            cur = fifo[head]
            head += 1
        else:
            cur = heapq.heappop(heap).node
        _, _, depth, h, (px, py), crates = nodes[cur]
        if len(crates) == len(lv.targets) and len(crates) > 0 and set(crates) == target_set:
            return True, actions(cur), h, False
        key = (px, py, crates)
        if key in visited:
            continue
        if best is None or h < nodes[best][3] or (h == nodes[best][3] and depth < nodes[best][2]):
            best = cur
        visited.add(key)
        for dx, dy in directions:
            nx, ny = px + dx, py + dy
            if lv.solid[ny][nx]:  # (the border is solid: no cell outside the level is ever asked for)
                continue
            ch, hh = crates, h
            if (nx, ny) in crates:
                bx, by = nx + dx, ny + dy
                if lv.solid[by][bx] or (bx, by) in crates:
                    continue
                k = crates.index((nx, ny))
                ch = crates[:k] + ((bx, by),) + crates[k + 1:]
                if any(c in lv.dead for c in ch):
                    continue
                hh = lv.heuristic(ch)
            nodes.append((cur, DIRECTIONS.index((dx, dy)), depth + 1, hh, (nx, ny), ch))
            if balance2 is None:
                fifo.append(len(nodes) - 1)
            else:
                heapq.heappush(heap, _Entry(2 * hh + balance2 * (depth + 1), len(nodes) - 1))
    dry = head >= len(fifo) if balance2 is None else len(heap) == 0
    return False, actions(best), nodes[best][3], dry


STAGES = (None, 2, 1, 0)  # BFS, A* with 2 * balance = 2, 1, 0


def solve(grid, power=10000, directions=DIRECTIONS, shortcut=True):
    """-> (moves, dist_win, stage): the reference's (solution, dist-win) of a map that meets the precondition and the index of
    the stage that won (0 BFS, 1..3 A* with balance 1, 0.5, 0; -1: none, moves == []).

    shortcut: a BFS stage that runs its queue dry without a win ends the cascade.  No stage can win then, and each A* stage
    would expand exactly the same set of states -- every reachable one -- and end with the smallest h of that set, which the
    BFS stage already holds; skipping them changes no answer, only the time."""
    lv = Level(grid)
    h = 0
    for i, b2 in enumerate(STAGES):
        won, moves, h, dry = _stage(lv, b2, power, directions)
        if won:
            return moves, 0, i
        if shortcut and i == 0 and dry:
            break
    return [], h, -1


def small_room(rng, shape, x_from=None):
    """the first family of the solver fixtures (oracle/gen_golden.py gen_stats_sokoban_solver): one room of 3..7 cells per side
    in a solid map, a few inner walls, one player and 1..3 crate / target pairs.  x_from: the least left edge of the room."""
    H, W = shape
    while True:
        g = np.full(shape, SOLID, np.uint8)
        h, w = int(rng.integers(3, min(8, H + 1))), int(rng.integers(3, min(8, W + 1)))
        y0 = int(rng.integers(0, H - h + 1))
        x0 = int(rng.integers(0 if x_from is None else max(0, min(x_from, W - w)), W - w + 1))
        g[y0:y0 + h, x0:x0 + w] = EMPTY
        for _ in range(int(rng.integers(0, 4))):
            g[y0 + int(rng.integers(h)), x0 + int(rng.integers(w))] = SOLID
        free = np.argwhere(g == EMPTY)
        k = int(rng.integers(1, 4))
        if len(free) < 1 + 2 * k:
            continue
        sel = free[rng.permutation(len(free))[: 1 + 2 * k]]
        for (y, x), t in zip(sel, [PLAYER] + [CRATE] * k + [TARGET] * k):
            g[y, x] = t
        return g
