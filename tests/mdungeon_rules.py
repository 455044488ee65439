"""MiniDungeon levels in plain Python: the rules MDungeonEvaluator's kernel implements, restated from the reference's text
(file:line relative to control_pcgrl/envs/): the statistics of MDungeonProblem.get_stats (probs/mdungeon/mdungeon_prob.py:151-171),
the game and the four searches of probs/mdungeon/mdungeon/engine.py, get_reward and get_episode_over.
tools/gen_golden_mdungeon.py pins it to the reference on every recorded level; the GPU tests compare the kernel with it on
generated levels.

A map is an integer array [H][W] of tile ids 0..7 (TILES); an id above 7 reads as solid (has_error says so).  Coordinates of
the game are those of the level with its solid border: x in 0..W + 1, y in 0..H + 1.

`wrong` names one deliberately wrong rule (WRONG_RULES) -- the generator checks that each fails some fixture.
"""
import heapq
import math

TILES = ["empty", "solid", "player", "exit", "potion", "treasure", "goblin", "ogre"]  # mdungeon_prob.py:50-51
EMPTY, SOLID, PLAYER, EXIT, POTION, TREASURE, GOBLIN, OGRE = range(8)
STAT_KEYS = ["player", "exit", "potions", "treasures", "enemies", "regions", "col-potions", "col-treasures", "col-enemies",
             "dist-win", "sol-length"]  # mdungeon_prob.py:153-165
DIRECTIONS = ((-1, 0), (1, 0), (0, -1), (0, 1))  # engine.py:3: left, right, up, down
STAGES = (1, 0.5, 0, None)  # mdungeon_prob.py:125-134: three A* balances, then the BFS
REWARD_ORDER = ("player", "exit", "enemies", "treasures", "potions", "regions", "col-enemies", "dist-win",
                "sol-length")  # mdungeon_prob.py:197-205
WEIGHTS = {"player": 3, "exit": 3, "potions": 1, "treasures": 1, "enemies": 2, "regions": 5, "col-enemies": 2, "dist-win": 0.1,
           "sol-length": 1}  # mdungeon_prob.py:32-42
PLAY_FIELDS = 12
MAX_ITEMS = 64  # the device's limit: a level that reaches the solver with more items is not searched (status 5)
MAX_HEALTH = 5  # engine.py:179, :236-237
DAMAGE = {GOBLIN: 1, OGRE: 2}  # engine.py:186-189
WRONG_RULES = ("fifo-ties", "key-without-health", "lost-not-counted", "potion-unclamped", "children-up-down-left-right",
               "blocked-no-child")


def clean(m):
    return [[int(t) if 0 <= int(t) < 8 else SOLID for t in row] for row in m]


def has_error(m):
    return any(not 0 <= int(t) < 8 for row in m for t in row)


def num_regions(m):
    """calc_num_regions (helper.py:200-210) over every tile but solid (mdungeon_prob.py:159)"""
    H, W = len(m), len(m[0])
    seen = [[m[y][x] == SOLID for x in range(W)] for y in range(H)]
    count = 0
    for y in range(H):
        for x in range(W):
            if seen[y][x]:
                continue
            count += 1
            todo = [(x, y)]
            seen[y][x] = True
            while todo:
                cx, cy = todo.pop()
                for nx, ny in ((cx - 1, cy), (cx + 1, cy), (cx, cy - 1), (cx, cy + 1)):
                    if 0 <= nx < W and 0 <= ny < H and not seen[ny][nx]:
                        seen[ny][nx] = True
                        todo.append((nx, ny))
    return count


class Level:
    """State.stringInitialize (engine.py:140-189) on _run_game's string (mdungeon_prob.py:101-120): the map inside a solid
    border; the three item lists in the scan's order, row-major"""

    def __init__(self, m):
        H, W = len(m), len(m[0])
        self.height, self.width = H + 2, W + 2
        self.solid = [[True] * (W + 2)] + [[True] + [t == SOLID for t in row] + [True] for row in m] + [[True] * (W + 2)]
        self.potions, self.treasures, self.enemies = [], [], []
        self.kind = {}  # (x, y) -> tile id of the item there
        self.start = self.door = None
        for y in range(H):
            for x in range(W):
                t, at = m[y][x], (x + 1, y + 1)
                if t == POTION:
                    self.potions.append(at)
                elif t == TREASURE:
                    self.treasures.append(at)
                elif t in (GOBLIN, OGRE):
                    self.enemies.append(at)
                elif t == PLAYER:
                    self.start = at
                elif t == EXIT:
                    self.door = at
                if t in (POTION, TREASURE, GOBLIN, OGRE):
                    self.kind[at] = t


class Node:
    """a search node with its game state; `left` is the frozenset of item cells still on the map"""
    __slots__ = ("x", "y", "health", "potions", "treasures", "enemies", "left", "depth", "parent", "action", "f", "blocked")

    def __lt__(self, other):  # engine.py:54-55
        return self.f < other.f

    @property
    def lost(self):  # engine.py:311-312
        return self.health <= 0


def heuristic(lv, n):
    """State.getHeuristic (engine.py:285-289)"""
    return abs(n.x - lv.door[0]) + abs(n.y - lv.door[1]) + 4 * (MAX_HEALTH - n.health) + 4 * -n.treasures


def won(lv, n):
    return (n.x, n.y) == lv.door  # engine.py:308-309


def child(lv, n, a, wrong=None):
    """State.update (engine.py:254-270) for direction a, then updatePlayer (engine.py:229-252).  The parent is neither won nor
    lost (such a node is never expanded), so checkOver's early return does not show."""
    dx, dy = DIRECTIONS[a]
    c = Node()
    c.parent, c.action, c.depth = n, a, n.depth + 1
    c.x, c.y, c.health, c.potions, c.treasures, c.enemies, c.left = n.x, n.y, n.health, n.potions, n.treasures, n.enemies, n.left
    x, y = n.x + dx, n.y + dy
    c.blocked = lv.solid[y][x]
    if c.blocked:
        return c
    c.x, c.y = x, y
    if (x, y) in n.left:
        t = lv.kind[(x, y)]
        c.left = n.left - {(x, y)}
        if t == POTION:  # counted and consumed even at full health
            c.potions += 1
            c.health += 2
            if c.health > MAX_HEALTH and wrong != "potion-unclamped":
                c.health = MAX_HEALTH
        elif t == TREASURE:
            c.treasures += 1
        else:
            c.enemies += 1
            c.health = max(0, c.health - DAMAGE[t])
    return c


def string_key(lv, n):
    """State.getKey's string (engine.py:272-283), built as it is there"""
    key = f"{n.x},{n.y},{n.health}|" + f"{lv.door[0]},{lv.door[1]}|"
    for p in lv.potions:
        if p in n.left:
            key += f"{p[0]},{p[1]},"
    key = key[:-1] + "|"
    for t in lv.treasures:
        if t in n.left:
            key += f"{t[0]},{t[1]},"
    key = key[:-1] + "|"
    for e in lv.enemies:
        if e in n.left:
            key += f"{e[0]},{e[1]},"
    return key[:-1]


def search(lv, balance, power, wrong=None, key_check=None, trace=None):
    """AStarAgent.getSolution (engine.py:105-129), or BFSAgent.getSolution (engine.py:61-81) with balance None.  Returns
    (returned node, won, iterations).  key_check: a dict; both keys of every tested node go in, and the two must agree one to
    one.  trace: a set that collects what happened."""
    root = Node()
    root.x, root.y = lv.start
    root.health, root.potions, root.treasures, root.enemies = MAX_HEALTH, 0, 0, 0
    root.left = frozenset(lv.potions + lv.treasures + lv.enemies)
    root.depth, root.parent, root.action, root.blocked = 0, None, None, False
    bfs = balance is None
    fifo = wrong == "fifo-ties" and not bfs
    root.f = 0 if bfs else heuristic(lv, root) + balance * 0
    queue, head, seq = [(root.f, 0, root) if fifo else root], 0, 0
    visited, best, best_h, iterations = set(), None, None, 0
    order = (2, 3, 0, 1) if wrong == "children-up-down-left-right" else (0, 1, 2, 3)
    while iterations < power and (head < len(queue) if bfs else queue):
        iterations += 1
        if bfs:
            cur = queue[head]  # pop(0): first in, first out
            head += 1
        elif fifo:
            cur = heapq.heappop(queue)[2]
        else:
            cur = heapq.heappop(queue)
        if cur.lost:
            if trace is not None:
                trace.add("lost-pop")
            if wrong == "lost-not-counted":
                iterations -= 1
            continue
        if won(lv, cur):
            return cur, True, iterations
        key = (cur.x, cur.y, cur.health, cur.left)
        if key_check is not None:
            s = string_key(lv, cur)
            assert key_check.setdefault(("t", key), s) == s and key_check.setdefault(("s", s), key) == key
            other = key_check.setdefault(("items", cur.left), cur.health)
            if other != cur.health and trace is not None:
                trace.add("same-items-two-healths")
        if wrong == "key-without-health":
            key = (cur.x, cur.y, cur.left)
        if key in visited:
            if trace is not None:
                trace.add("visited-pop")
            continue
        h = heuristic(lv, cur)
        if best is None or h < best_h:
            best, best_h = cur, h
        elif h == best_h and cur.depth < best.depth:
            best = cur
        visited.add(key)
        for a in order:
            c = child(lv, cur, a, wrong)
            if trace is not None:
                if c.blocked:
                    trace.add("wall")
                elif (c.x, c.y) in cur.left:
                    t = lv.kind[(c.x, c.y)]
                    if t == POTION and cur.health == 5:
                        trace.add("potion-at-5")
                    if t == POTION and cur.health == 4:
                        trace.add("potion-from-4")
                    if t == OGRE and cur.health == 1:
                        trace.add("ogre-at-1")
            if c.blocked and wrong == "blocked-no-child":
                continue
            if bfs:
                queue.append(c)
            else:
                c.f = heuristic(lv, c) + balance * c.depth
                if fifo:
                    seq += 1
                    heapq.heappush(queue, (c.f, seq, c))
                else:
                    heapq.heappush(queue, c)
    if trace is not None and iterations < power:
        trace.add("emptied")
    return best, False, iterations


def actions(n):
    out = []
    while n.parent is not None:
        out.insert(0, n.action)
        n = n.parent
    return out


def run_game(m, power, wrong=None, key_check=None, trace=None, stages=None):
    """_run_game (mdungeon_prob.py:100-138).  Returns (dist-win, sol-length, returned node, stage that won or 0, [iterations of
    the four stages], level).  stages: a list that receives [x, y, depth] of the node each stage returned."""
    lv = Level(m)
    its = [0, 0, 0, 0]
    node = None
    for stage, balance in enumerate(STAGES):
        node, ok, its[stage] = search(lv, balance, power, wrong, key_check, trace)
        if stages is not None:
            stages.append([node.x, node.y, node.depth])
        if ok:
            return 0, node.depth, node, stage + 1, its, lv
    return heuristic(lv, node), 0, node, 0, its, lv


def outputs(m, power, cap=0, wrong=None, key_check=None, trace=None, stages=None):
    """What the device writes for one level: (stats [11], moves [cap], length, play [12]), include/pcgrl_amd_mdungeon.h"""
    m = clean(m)
    H, W = len(m), len(m[0])
    count = [sum(row.count(t) for row in m) for t in range(8)]
    stats = [count[PLAYER], count[EXIT], count[POTION], count[TREASURE], count[GOBLIN] + count[OGRE], num_regions(m), 0, 0, 0,
             W * H, 0]
    play = [-1] + [0] * 11
    moves, length = [-1] * cap, 0
    if stats[0] == 1 and stats[1] == 1 and stats[5] == 1:  # mdungeon_prob.py:166
        if stats[2] + stats[3] + stats[4] > MAX_ITEMS:
            play[0] = 5
        else:
            stats[9], stats[10], node, stage, its, lv = run_game(m, power, wrong, key_check, trace, stages)
            stats[6], stats[7], stats[8] = node.potions, node.treasures, node.enemies
            acts = actions(node)
            length = len(acts)
            moves = (acts + [-1] * cap)[:cap]
            play = [stage] + its + [node.x, node.y, node.health, node.potions, node.treasures, node.enemies, node.depth]
    return stats, moves, length, play


def get_stats(m, power, wrong=None):
    return outputs(m, power, 0, wrong)[0]


def range_reward(new, old, low, high):
    """get_range_reward (helper.py:550-560)"""
    if low <= new <= high and low <= old <= high:
        return 0
    if old <= high and new <= high:
        return min(new, low) - min(old, low)
    if old >= low and new >= low:
        return max(old, high) - max(new, high)
    if new > high and old < low:
        return high - new + old - low
    if new < low and old > high:
        return high - old + new - low
    raise AssertionError("unreachable")


def reward(new, old, weights=None, max_enemies=6, max_potions=2, max_treasures=3):
    """get_reward (mdungeon_prob.py:183-205) of two statistics lists"""
    w = dict(WEIGHTS)
    w.update(weights or {})
    inf = math.inf
    bounds = {"player": (1, 1), "exit": (1, 1), "potions": (-inf, max_potions), "treasures": (-inf, max_treasures),
              "enemies": (1, max_enemies), "regions": (1, 1), "col-enemies": (inf, inf), "dist-win": (-inf, -inf),
              "sol-length": (inf, inf)}
    total = None
    for k in REWARD_ORDER:
        j = STAT_KEYS.index(k)
        term = range_reward(int(new[j]), int(old[j]), *bounds[k]) * w[k]
        total = term if total is None else total + term
    return total


def episode_over(stats, target_col_enemies=0.5, target_solution=20):
    """get_episode_over (mdungeon_prob.py:218-221)"""
    return bool(stats[10] >= target_solution and stats[4] > 0 and stats[8] / max(1, stats[4]) > target_col_enemies)
