"""What LodeRunnerEvaluator.routes() has to return, stated on the host: from the plain-Python rules
(tests/loderunner_rules.py: play(m, record=...)) and from the fixtures recorded from the reference
(tools/gen_golden_loderunner_routes.py -> tests/golden/loderunner_routes).  Test infrastructure, shared by
tests/test_loderunner_routes_cpu.py, tests/test_gpu_loderunner_routes.py and tools/loderunner_routes_bench.py.

A pair is (gold index in row-major order, to_goal, to_start), each of the two (cells, moves) as the reference's Node.get_path
lists them: from the goal back to the source.  The routes run the other way."""
import numpy as np

import loderunner_levels as LL
import loderunner_rules as R

GOLD_KIND_SEED = 1  # loderunner_levels.batch("gold", 1, 300, 8, 12): 152 levels with a route, 6 with a counted gold at index >= 32


def pairs_of_rules(m):
    """the counted pairs of one map by the rules, in gold order"""
    stats, rec = R.get_stats(m)
    if rec is None:
        return []
    record = []
    R.play(m, record=record)
    index = {g: j for j, g in enumerate(rec["golds"])}
    return [(index[g], a, b) for g, a, b in record if b is not None]


def pairs_of_fixture(z, i):
    """the recorded pairs of level i of a fixture set (moves as numbers)"""
    out = []
    for p in np.flatnonzero(z["pair_level"] == i):
        both = []
        for k in (2 * p, 2 * p + 1):
            cells = [tuple(int(v) for v in c) for c in z["path_cells"][z["path_off"][k]:z["path_off"][k + 1]]]
            moves = [int(a) for a in z["path_actions"][z["act_off"][k]:z["act_off"][k + 1]]]
            both.append((cells, moves))
        out.append((int(z["pair_gold"][p]), both[0], both[1]))
    return out


def serpentine(h, w):
    """brick floors under every second row, ladders at alternating ends, the player at the bottom left end and one gold at the
    far end of the top row: one way through, every walkable cell on it"""
    m = np.zeros((h, w), dtype=np.uint8)
    m[1::2, :] = LL.BRICK
    m[h - 1, :] = LL.BRICK
    rows = list(range(h - 2, -1, -2))  # the walkable rows, bottom up
    for k, r in enumerate(rows[:-1]):
        c = w - 1 if k % 2 == 0 else 0
        m[r - 1:r + 1, c] = LL.LADDER
    m[rows[0], 0] = LL.PLAYER
    m[rows[-1], w - 1 if len(rows) % 2 else 0] = LL.GOLD
    return m


def expect(pairs_per_level, gold_cap, route_cap, moves=True):
    """coords, moves, tour_len, gold_off, gold_back as the ABI defines them, from the pairs of every level"""
    n = len(pairs_per_level)
    out = {"tour_len": np.zeros(n, np.int32), "coords": np.full((n, route_cap, 2), -1, np.int16)}
    if moves:
        out["moves"] = np.full((n, route_cap), -1, np.int8)
    if gold_cap:
        out["gold_off"] = np.full((n, gold_cap), -1, np.int32)
        out["gold_back"] = np.zeros((n, gold_cap), np.int16)
    for i, pairs in enumerate(pairs_per_level):
        cells, taken = [], []
        for j, to_goal, to_start in pairs:
            if j < gold_cap:
                out["gold_off"][i, j] = len(cells)
                out["gold_back"][i, j] = len(to_start[0])
            for path, mv in (to_goal, to_start):
                assert len(mv) == len(path) - 1
                cells += path[::-1]
                taken += list(mv[::-1]) + [-1]
        out["tour_len"][i] = len(cells)
        k = min(len(cells), route_cap)
        if k:
            out["coords"][i, :k] = cells[:k]
            if moves:
                out["moves"][i, :k] = taken[:k]
    return out


def split(pairs):
    """what split_routes returns for a level with these pairs"""
    return [(a[0][0], a[0][::-1], b[0][::-1]) for _, a, b in pairs]
