"""Dangerous Dave levels in plain Python: the rules DDaveEvaluator's kernel implements, restated from the reference's text
(file:line relative to control_pcgrl/envs/): the statistics of DDaveProblem.get_stats (probs/ddave/ddave_prob.py:149-169), the
game and the four searches of probs/ddave/ddave/engine.py, get_reward and get_episode_over.  tools/gen_golden_ddave.py pins it
to the reference on every recorded level; the GPU tests compare the kernel with it on generated levels.

A map is an integer array [H][W] of tile ids 0..6 (TILES); an id above 6 reads as solid (has_error says so).  Coordinates of
the game are those of the level with its solid border: x in 0..W + 1, y in 0..H + 1.

`wrong` names one deliberately wrong rule (WRONG_RULES) -- the generator checks that each fails some fixture.
"""
import heapq
import math

TILES = ["empty", "solid", "player", "exit", "diamond", "key", "spike"]  # ddave_prob.py:53-54
EMPTY, SOLID, PLAYER, EXIT, DIAMOND, KEY, SPIKE = range(7)
STAT_KEYS = ["player", "dist-floor", "exit", "diamonds", "key", "spikes", "regions", "num-jumps", "col-diamonds", "dist-win",
             "sol-length"]  # ddave_prob.py:151-163
DIRECTIONS = ((0, 0), (-1, 0), (1, 0), (0, -1))  # engine.py:3
STAGES = (1, 0.5, 0, None)  # ddave_prob.py:122-131: three A* balances, then the BFS
REWARD_ORDER = ("player", "dist-floor", "exit", "spikes", "diamonds", "key", "regions", "num-jumps", "dist-win",
                "sol-length")  # ddave_prob.py:196-205
WEIGHTS = {"player": 3, "dist-floor": 2, "exit": 3, "diamonds": 1, "key": 3, "spikes": 1, "regions": 5, "num-jumps": 3,
           "dist-win": 0.1, "sol-length": 1}  # ddave_prob.py:31-42
PLAY_FIELDS = 12
MAX_DIAMONDS = 64  # the device's limit: a level that reaches the solver with more is not searched (status 5)
WRONG_RULES = ("fifo-ties", "key-with-airtime", "best-without-depth", "unbordered-heuristic", "lost-not-counted")


def clean(m):
    return [[int(t) if 0 <= int(t) < 7 else SOLID for t in row] for row in m]


def has_error(m):
    return any(not 0 <= int(t) < 7 for row in m for t in row)


def dist_floor(m):
    """get_floor_dist(map, ["player"], ["solid"]) (helper.py:40-65): per player tile dy - 1 of the first solid tile at or
    below it, H - 1 when the column has none; summed; no border"""
    H, total = len(m), 0
    for y in range(H):
        for x in range(len(m[0])):
            if m[y][x] != PLAYER:
                continue
            d = H - 1
            for dy in range(H - y):
                if m[y + dy][x] == SOLID:
                    d = dy - 1
                    break
            total += d
    return total


def num_regions(m):
    """calc_num_regions (helper.py:200-210) over empty, player, diamond, key, exit: spikes and solids separate"""
    H, W = len(m), len(m[0])
    seen = [[m[y][x] in (SOLID, SPIKE) for x in range(W)] for y in range(H)]
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
    """State.stringInitialize (engine.py:140-187) on _run_game's string (ddave_prob.py:100-115): the map inside a solid border"""

    def __init__(self, m):
        H, W = len(m), len(m[0])
        self.height, self.width = H + 2, W + 2
        self.solid = [[True] * (W + 2)] + [[True] + [t == SOLID for t in row] + [True] for row in m] + [[True] * (W + 2)]
        self.spikes, self.diamonds = [], []  # in the scan's order: row-major
        self.start = self.door = self.key = None
        for y in range(H):
            for x in range(W):
                t, at = m[y][x], (x + 1, y + 1)
                if t == DIAMOND:
                    self.diamonds.append(at)
                elif t == SPIKE:
                    self.spikes.append(at)
                elif t == PLAYER:
                    self.start = at
                elif t == EXIT:
                    self.door = at
                elif t == KEY:
                    self.key = at
        self.spike_set = set(self.spikes)
        self.h_width, self.h_height = self.width, self.height  # what getHeuristic adds while the key is on the map


class Node:
    """a search node with its game state; `left` is the tuple of diamonds still on the map, in list order"""
    __slots__ = ("x", "y", "air", "key", "lost", "jumps", "left", "depth", "parent", "action", "f", "cut")

    def __lt__(self, other):  # engine.py:54-55
        return self.f < other.f


def heuristic(lv, n):
    """State.getHeuristic (engine.py:278-283)"""
    if n.key:
        d = abs(n.x - lv.door[0]) + abs(n.y - lv.door[1])
    else:
        d = abs(n.x - lv.key[0]) + abs(n.y - lv.key[1]) + (lv.h_width + lv.h_height)
    return d + 5 * -(len(lv.diamonds) - len(n.left))


def won(lv, n):
    return n.key and (n.x, n.y) == lv.door  # engine.py:304-305


def child(lv, n, a):
    """State.update (engine.py:229-264) for direction a, then updatePlayer (engine.py:212-227)"""
    dx, dy = DIRECTIONS[a]
    c = Node()
    c.parent, c.action, c.depth, c.cut = n, a, n.depth + 1, False
    x, y, air, jumps = n.x, n.y, n.air, n.jumps
    ground, ceiling = lv.solid[y + 1][x], lv.solid[y - 1][x]
    if dx != 0:  # a horizontal move leaves the jump out (elif)
        if not lv.solid[y][x + dx]:
            x += dx
    elif dy == -1:
        if ground and not ceiling:
            air = 3
            jumps += 1
    if air > 1:
        air -= 1
        if not lv.solid[y - 1][x]:
            y -= 1
        else:
            air = 1  # the jump is cut short
            c.cut = True
    elif air == 1:
        air = 0
    elif not lv.solid[y + 1][x]:
        y += 1
    c.x, c.y, c.air, c.jumps, c.key, c.lost, c.left = x, y, air, jumps, n.key, False, n.left
    if (x, y) in n.left:  # a diamond first, and nothing else then
        c.left = tuple(d for d in n.left if d != (x, y))
    elif (x, y) in lv.spike_set:
        c.lost = True
    elif not n.key and (x, y) == lv.key:
        c.key = True
    return c


def string_key(lv, n):
    """State.getKey's string (engine.py:266-276), built as it is there"""
    key = f"{n.x},{n.y},{0 if n.lost else 1}|" + f"{lv.door[0]},{lv.door[1]}|"
    if not n.key:
        key += f"{lv.key[0]},{lv.key[1]}|"
    for d in n.left:
        key += f"{d[0]},{d[1]},"
    key = key[:-1] + "|"
    for s in lv.spikes:
        key += f"{s[0]},{s[1]},"
    return key[:-1]


def search(lv, balance, power, wrong=None, key_check=None, trace=None):
    """AStarAgent.getSolution (engine.py:105-129), or BFSAgent.getSolution (engine.py:61-81) with balance None.  Returns
    (returned node, won, iterations).  key_check: a dict; both keys of every tested node go in, and the two must agree.
    trace: a set that collects what happened ("lost-pop", "visited-pop", "ceiling", "cut-short", "emptied")."""
    root = Node()
    root.x, root.y = lv.start
    root.air, root.key, root.lost, root.jumps, root.left = 0, False, False, 0, tuple(lv.diamonds)
    root.depth, root.parent, root.action, root.cut = 0, None, None, False
    bfs = balance is None
    root.f = 0 if bfs else heuristic(lv, root) + balance * 0
    queue, head, seq = [(root.f, 0, root) if wrong == "fifo-ties" and not bfs else root], 0, 0
    visited, best, best_h, iterations = set(), None, None, 0
    while iterations < power and (head < len(queue) if bfs else queue):
        iterations += 1
        if bfs:
            cur = queue[head]  # pop(0): first in, first out
            head += 1
        elif wrong == "fifo-ties":
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
        key = (cur.x, cur.y, cur.key, frozenset(cur.left))
        if wrong == "key-with-airtime":
            key += (cur.air,)
        if key_check is not None:
            s = string_key(lv, cur)
            assert key_check.setdefault(("t", key), s) == s and key_check.setdefault(("s", s), key) == key
        if key in visited:
            if trace is not None:
                trace.add("visited-pop")
            continue
        h = heuristic(lv, cur)
        if best is None or h < best_h:
            best, best_h = cur, h
        elif h == best_h and cur.depth < best.depth and wrong != "best-without-depth":
            best = cur
        visited.add(key)
        for a in range(4):
            c = child(lv, cur, a)
            if trace is not None:
                if a == 3 and lv.solid[cur.y + 1][cur.x] and lv.solid[cur.y - 1][cur.x]:
                    trace.add("ceiling")
                if c.cut:
                    trace.add("cut-short")
            if bfs:
                queue.append(c)
            else:
                c.f = heuristic(lv, c) + balance * c.depth
                if wrong == "fifo-ties":
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
    """_run_game (ddave_prob.py:100-135).  Returns (dist-win, sol-length, returned node, stage that won or 0, [iterations of
    the four stages], level).  stages: a list that receives [x, y, depth] of the node each stage returned."""
    lv = Level(m)
    if wrong == "unbordered-heuristic":
        lv.h_width, lv.h_height = lv.width - 2, lv.height - 2
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
    """What the device writes for one level: (stats [11], moves [cap], length, play [12]), include/pcgrl_amd_ddave.h"""
    m = clean(m)
    H, W = len(m), len(m[0])
    count = [sum(row.count(t) for row in m) for t in range(7)]
    stats = [count[PLAYER], dist_floor(m), count[EXIT], count[DIAMOND], count[KEY], count[SPIKE], num_regions(m), 0, 0, W * H, 0]
    play = [-1] + [0] * 10 + [0]
    play[10] = count[DIAMOND]
    moves, length = [-1] * cap, 0
    if stats[0] == 1 and stats[2] == 1 and stats[4] == 1 and stats[6] == 1:  # ddave_prob.py:164-165
        if count[DIAMOND] > MAX_DIAMONDS:
            play[0] = 5
        else:
            stats[9], stats[10], node, stage, its, lv = run_game(m, power, wrong, key_check, trace, stages)
            stats[7], stats[8] = node.jumps, len(lv.diamonds) - len(node.left)
            acts = actions(node)
            length = len(acts)
            moves = (acts + [-1] * cap)[:cap]
            play = [stage] + its + [node.x, node.y, node.air, 0 if node.lost else 1, int(node.key), count[DIAMOND], node.depth]
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


def reward(new, old, weights=None, max_diamonds=3, min_spikes=10):
    """get_reward (ddave_prob.py:181-205) of two statistics lists"""
    w = dict(WEIGHTS)
    w.update(weights or {})
    inf = math.inf
    bounds = {"player": (1, 1), "exit": (1, 1), "diamonds": (-inf, max_diamonds), "dist-floor": (0, 0), "key": (1, 1),
              "spikes": (min_spikes, inf), "regions": (1, 1), "num-jumps": (inf, inf), "dist-win": (-inf, -inf),
              "sol-length": (inf, inf)}
    total = None
    for k in REWARD_ORDER:
        j = STAT_KEYS.index(k)
        term = range_reward(int(new[j]), int(old[j]), *bounds[k]) * w[k]
        total = term if total is None else total + term
    return total


def episode_over(stats, target_jumps=2, target_solution=20):
    """get_episode_over (ddave_prob.py:218-220)"""
    return bool(stats[10] >= target_solution and stats[7] > target_jumps)
