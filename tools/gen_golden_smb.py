"""Super Mario Bros levels, recorded from the REFERENCE on the CPU (through oracle/ref_env.py) -> tests/golden/smb/*.npz.
Data only; needs the reference tree; a few minutes on one core.  Not for the GPU machine.

    python tools/gen_golden_smb.py

Per set (one file: a map shape, a solver_power, levels of tests/smb_levels.py) and per level:
  grids        uint8 [n][H][W]
  stats        int32 [n][9]: SMBCtrlProblem.get_stats(map), in its dict order (`stat_keys`)
  loss, loss_alt   float64 [n]: env.metrics = the statistics on a make_env narrow env, ControlWrapper.get_loss() -- with the
               default weights and with `alt_weights` (dyadic values: all_metrics is a set, so the order of the sum is not
               fixed, and only sums that are exact in every order can be compared bit for bit)
  p<k>_*       pass k = 1, 2: AStarAgent.getSolution(state, balance 1 / 0, solver_power) called directly on the State
               _run_game builds (both passes for every level, whether pass 1 wins or not): moves int8 [n][L] (-1 past the
               end), length, iterations, won, final int32 [n][4] = x, y, airTime, jumps, jump_locs int16 [n][J][2] (-1 past the
               end)
  kind         which generator made the level;  solver_power;  trg_lo / trg_hi / weights: the wrapper's frozen tables

The script fails unless tests/smb_rules.py reproduces every recorded field and the set holds each case listed in CASES.
One case of the issue cannot exist: a lose node.  checkLose is y >= height, and the only move that increases y needs
checkMovableLocation(x, y + 1), which is false for y + 1 >= height -- the player stands on the bottom row of a floor gap
instead of falling out.  The script counts checkLose() == True over every reference search and asserts the count is 0, and
asserts the gap case as "the final node stands in a floor gap's column or passed one".
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import smb_levels as sl  # noqa: E402
import smb_rules as R  # noqa: E402
import ref_env  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "smb")
ALT_WEIGHTS = {"dist-floor": 0.5, "disjoint-tubes": 3, "enemies": 0.25, "empty": 2, "noise": 1, "jumps": 8, "jumps-dist": 0,
               "dist-win": 1.5, "sol-length": 4}
# name: (H, W, solver_power, [(kind, seed), ...]); "flat" is a structured level with nothing on the floor
SETS = {
    "stock_p10000": (16, 116, 10000, [("structured", s) for s in range(4)] + [("random", s) for s in range(3)]
                     + [("walled", s) for s in range(2)] + [("flat", 0)]),
    "stock_p1000": (16, 116, 1000, [("structured", s) for s in (0, 7, 12)] + [("random", 2), ("walled", 3)]),
    "stock_p300": (16, 116, 300, [("structured", 1), ("random", 1), ("walled", 0)]),
    "wide128_p10000": (16, 128, 10000, [("structured", 0), ("random", 1), ("walled", 0)]),
    "w65_p10000": (16, 65, 10000, [("structured", 0), ("random", 0), ("walled", 1)]),
    "w64_p300": (16, 64, 300, [("structured", 0), ("random", 0)]),
    "h16w24_p10000": (16, 24, 10000, [(k, s) for k in sl.KINDS for s in range(3)]),
    "h8w30_p10000": (8, 30, 10000, [(k, s) for k in sl.KINDS for s in (0, 18)]),
    "h11w40_p300": (11, 40, 300, [(k, s) for k in sl.KINDS for s in range(2)]),
    "h5w7_p10000": (5, 7, 10000, [(k, s) for k in sl.KINDS for s in range(3)]),
    "h4w5_p10000": (4, 5, 10000, [(k, s) for k in sl.KINDS for s in range(2)]),
    "h4w1_p10000": (4, 1, 10000, [("structured", 0), ("random", 1)]),
}
CASES = ["win in pass 1", "win in pass 2 only", "both passes on the cap", "open list emptied without a win",
         "player above row 0", "floor gap crossed", "no jump", "enemy with no floor below", "tube width 1", "tube width 2",
         "tube width 3"]


def make_level(kind, seed, h, w):
    if kind == "flat":
        return sl.structured(np.random.default_rng(seed), h, w, 0.0, 0.0, 0.0, 0.0)
    return sl.make(kind, seed, h, w)


class Recorder:
    """One reference env per map shape; the State of _run_game is caught by wrapping AStarAgent.getSolution."""

    def __init__(self, h, w, power):
        from control_pcgrl.envs.probs.smb.smb import engine
        self.engine = engine
        self.envs = {}
        for name, weights in (("default", dict(R.DEFAULT_WEIGHTS)), ("alt", dict(ALT_WEIGHTS))):
            env = ref_env.make_reference_env(ref_env.make_cfg("smb", "narrow", (h, w), weights=weights))
            cw = env
            while type(cw).__name__ != "ControlWrapper":
                cw = cw.env
            self.envs[name] = cw
        self.prob = self.envs["default"].unwrapped._prob
        assert type(self.prob).__name__ == "SMBCtrlProblem" and (self.prob._height, self.prob._width) == (h, w)
        self.prob._solver_power = power
        self.tiles = self.prob.get_tile_types()
        self.lose_seen = 0

    def level(self, m):
        engine = self.engine
        caught = []
        orig_solution, orig_lose = engine.AStarAgent.getSolution, engine.State.checkLose
        rec = self

        def catching(agent, state, balance=1, maxIterations=-1):
            caught.append(state)
            return orig_solution(agent, state, balance, maxIterations)

        def counting(state):
            lost = orig_lose(state)
            rec.lose_seen += bool(lost)
            return lost

        engine.AStarAgent.getSolution, engine.State.checkLose = catching, counting
        try:
            stats = self.prob.get_stats([[self.tiles[t] for t in row] for row in m])
            passes = []
            for balance in (1, 0):
                sol, node, iters = orig_solution(engine.AStarAgent(), caught[0], balance, self.prob._solver_power)
                pl = node.state.player
                passes.append({"moves": [engine.directions.index(d) for d in sol], "iterations": iters,
                               "won": int(node.checkWin()), "final": [pl["x"], pl["y"], pl["airTime"], pl["jumps"]],
                               "jump_locs": [tuple(l) for l in pl["jump_locs"]]})
        finally:
            engine.AStarAgent.getSolution, engine.State.checkLose = orig_solution, orig_lose
        assert list(stats) == R.STAT_KEYS, list(stats)
        losses = {}
        for name, cw in self.envs.items():
            cw.metrics = stats
            losses[name] = float(cw.get_loss())
        return [int(stats[k]) for k in R.STAT_KEYS], passes, losses


def pad(rows, width, fill=-1, dtype=np.int8, inner=()):
    out = np.full((len(rows), max(width, 1)) + inner, fill, dtype=dtype)
    for i, r in enumerate(rows):
        if len(r):
            out[i, :len(r)] = np.asarray(r, dtype=dtype).reshape((len(r),) + inner)
    return out


def cases_of(m, power, stats, passes):
    """Which of CASES this level shows."""
    h, w = m.shape
    got = set()
    p1, p2 = passes
    if p1["won"]:
        got.add("win in pass 1")
    elif p2["won"]:
        got.add("win in pass 2 only")
    elif p1["iterations"] == power and p2["iterations"] == power:
        got.add("both passes on the cap")
    elif p2["iterations"] < power:
        got.add("open list emptied without a win")
    final = p1 if p1["won"] else p2
    solid, ex, x, y = R.build_level(m)
    air, ys, xs = 0, [y], [x]
    for a in final["moves"]:
        x, y, air, _ = R.move(solid, x, y, air, a)
        ys.append(y)
        xs.append(x)
    if min(ys) < 0:
        got.add("player above row 0")
    gap_cols = [c + 3 for c in range(w) if m[h - 1, c] in (0, 2, 5) and m[h - 2, c] in (0, 2, 5)]
    if gap_cols and max(xs) > min(gap_cols):
        got.add("floor gap crossed")
    if final["final"][3] == 0:
        got.add("no jump")
    for yy, xx in zip(*np.nonzero(m == 2)):
        if not np.isin(m[yy + 1:, xx], R.FLOOR).any():
            got.add("enemy with no floor below")
    for row in m:
        run = 0
        for t in list(row) + [0]:
            if t == 6:
                run += 1
            else:
                if 1 <= run <= 3:
                    got.add(f"tube width {run}")
                run = 0
    return got


def main():
    assert ref_env.available(), "the reference tree is needed"
    os.makedirs(OUT, exist_ok=True)
    seen_cases, total, lose_seen = {}, 0, 0
    for name, (h, w, power, levels) in SETS.items():
        rec = Recorder(h, w, power)
        grids, stats, kinds, loss, loss_alt = [], [], [], [], []
        per_pass = [[], []]
        for kind, seed in levels:
            m = make_level(kind, seed, h, w)
            st, passes, losses = rec.level(m)
            # the rules reproduce every recorded field
            r_st, r_rec = R.get_stats(m, power)
            assert r_st == st, (name, kind, seed, r_st, st)
            for k, balance in enumerate((1, 0)):
                rp = R.run_pass(m, balance, power)
                ref = passes[k]
                assert (rp["moves"], rp["iterations"], rp["won"], [rp["x"], rp["y"], rp["air"], rp["jumps"]], rp["jump_locs"]) == \
                    (ref["moves"], ref["iterations"], ref["won"], ref["final"], ref["jump_locs"]), (name, kind, seed, k)
            assert R.loss(st) == losses["default"] and R.loss(st, ALT_WEIGHTS) == losses["alt"], (name, kind, seed, losses)
            for c in cases_of(m, power, st, passes):
                seen_cases.setdefault(c, []).append(f"{name}:{kind}{seed}")
            grids.append(m)
            stats.append(st)
            kinds.append(kind)
            loss.append(losses["default"])
            loss_alt.append(losses["alt"])
            for k in range(2):
                per_pass[k].append(passes[k])
        lose_seen += rec.lose_seen
        cw = rec.envs["default"]
        arrays = {
            "grids": np.stack(grids).astype(np.uint8), "stats": np.asarray(stats, dtype=np.int32), "kind": np.asarray(kinds),
            "stat_keys": np.asarray(R.STAT_KEYS), "solver_power": np.int32(power),
            "loss": np.asarray(loss, dtype=np.float64), "loss_alt": np.asarray(loss_alt, dtype=np.float64),
            "weights": np.asarray([float(cw.metric_weights[k]) for k in R.STAT_KEYS]),
            "alt_weights": np.asarray([float(ALT_WEIGHTS[k]) for k in R.STAT_KEYS]),
            "trg_lo": np.asarray([float(t[0] if isinstance(t, tuple) else t) for t in (cw.static_trgs[k] for k in R.STAT_KEYS)]),
            "trg_hi": np.asarray([float(t[1] if isinstance(t, tuple) else t) for t in (cw.static_trgs[k] for k in R.STAT_KEYS)]),
        }
        for k in range(2):
            ps = per_pass[k]
            arrays[f"p{k + 1}_moves"] = pad([p["moves"] for p in ps], max(len(p["moves"]) for p in ps))
            arrays[f"p{k + 1}_length"] = np.asarray([len(p["moves"]) for p in ps], dtype=np.int32)
            arrays[f"p{k + 1}_iterations"] = np.asarray([p["iterations"] for p in ps], dtype=np.int32)
            arrays[f"p{k + 1}_won"] = np.asarray([p["won"] for p in ps], dtype=np.int32)
            arrays[f"p{k + 1}_final"] = np.asarray([p["final"] for p in ps], dtype=np.int32)
            arrays[f"p{k + 1}_jump_locs"] = pad([p["jump_locs"] for p in ps], max(len(p["jump_locs"]) for p in ps),
                                               dtype=np.int16, inner=(2,))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size <= 100 * 1024, (path, size)
        total += size
        print(f"{name}: {len(levels)} levels, {size} bytes", flush=True)
    assert total <= 300 * 1024, total
    for c in CASES:
        assert seen_cases.get(c), f"no level shows: {c}"
        print(f"{c}: {len(seen_cases[c])} levels, e.g. {seen_cases[c][0]}")
    assert lose_seen == 0, lose_seen  # see the module docstring
    print("checkLose() was never true;", total, "bytes in all")


if __name__ == "__main__":
    main()
