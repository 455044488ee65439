"""Super Mario Bros episodes, recorded from the REFERENCE on the CPU (through oracle/ref_env.py) -> tests/golden/smb_env/*.npz.
Data only; needs the reference tree; a few minutes on one core.  Not for the GPU machine.

    python tools/gen_golden_smb_env.py

One file per episode run (EPISODES): make_env(cfg) of the reference for smb + narrow / turtle, seeded once, stepped `steps`
times; when a step ends an episode the env is reset (its streams continue) and the step's observation and position are the new
episode's first, as SmbVecEnv reports them with auto_reset.  Arrays, T = steps:
  representation, map_shape [2], obs_window [2], seed, solver_power, max_board_scans, change_percentage (-1 = none),
  max_iterations, max_changes (-1 = none), weights [9] (stat_keys order), stat_keys
  actions      int32 [T]
  pos          int32 [T][2]   (row, col) after the step (after the reset when the step ended an episode)
  stats        int32 [T][9]   the env's _rep_stats after the step (of the finished episode where one ended)
  reward       float64 [T]    ControlWrapper's loss - last_loss
  done         uint8 [T]
  iteration, changes  int32 [T]  (of the finished episode where one ended)
  obs_crc      uint32 [T]     zlib.crc32 of the uint8 observation [oh][ow][8]
  pos0, stats0, obs0_crc      the same after the first reset
  full_steps   int32 [K]      -1 (the first reset), 0, T - 1 and every step after an episode end
  full_map     uint8 [K][H][W], full_obs uint8 [K][oh][ow][8]   the map and the observation after those steps

The script fails unless tests/smb_env_rules.py reproduces every recorded field, and unless the set shows each case of CASES.
"""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import smb_levels as sl  # noqa: E402
import smb_rules as R  # noqa: E402
import smb_env_rules as E  # noqa: E402
import ref_env  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "smb_env")
ALT_WEIGHTS = {"dist-floor": 0.5, "disjoint-tubes": 3, "enemies": 0.25, "empty": 2, "noise": 1, "jumps": 8, "jumps-dist": 0,
               "dist-win": 1.5, "sol-length": 4}  # dyadic, as tools/gen_golden_smb.py: exact in every order of the sum
# name: representation, (H, W), seed, steps, solver_power, extras
EPISODES = {
    "narrow_4x5": ("narrow", (4, 5), 11, 140, 10000, {}),
    "turtle_5x7_cp02": ("turtle", (5, 7), 12, 150, 10000, {"change_percentage": 0.2}),
    "narrow_8x20_p300": ("narrow", (8, 20), 13, 200, 300, {}),
    "turtle_8x20_p300": ("turtle", (8, 20), 14, 200, 300, {}),
    "narrow_6x12_win5x9": ("narrow", (6, 12), 15, 120, 10000, {"obs_window": (5, 9)}),
    "turtle_5x7_alt": ("turtle", (5, 7), 16, 120, 10000, {"weights": ALT_WEIGHTS}),
    "paint_8x30_p300": ("narrow", (8, 30), 17, 0, 300, {"paint": ("structured", 0), "edits": 40}),
    "paint_6x70_p300": ("narrow", (6, 70), 18, 0, 300, {"paint": ("structured", 1), "edits": 40}),
    "narrow_16x116": ("narrow", (16, 116), 19, 120, 10000, {}),
    "turtle_16x116": ("turtle", (16, 116), 20, 120, 10000, {}),
    "narrow_16x127": ("narrow", (16, 127), 21, 20, 10000, {}),
}
CASES = ["win in pass 1", "win in pass 2 only or both passes on the cap", "edit that kept solidity", "no-change step",
         "done by iterations", "done by changes", "automatic reset"]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes()) & 0xFFFFFFFF


def record(name, rep, shape, seed, steps, power, extra, seen):
    h, w = shape
    weights = dict(extra.get("weights", R.DEFAULT_WEIGHTS))
    cp = extra.get("change_percentage")
    window = extra.get("obs_window")
    cfg = ref_env.make_cfg("smb", rep, shape, obs_window=window, weights=dict(weights), change_percentage=cp)
    env = ref_env.make_reference_env(cfg, seed=seed)
    u = env.unwrapped
    assert type(u._prob).__name__ == "SMBCtrlProblem"
    u._prob._solver_power = power
    rules = E.SmbEnvRules(rep, shape, seed=seed, obs_window=window, weights=weights, change_percentage=cp, solver_power=power)
    assert (u._max_iterations, u._max_changes) == (rules.max_iterations, rules.max_changes)
    arng = np.random.default_rng(1000 + seed)
    if "paint" in extra:
        level = sl.make(extra["paint"][0], extra["paint"][1], h, w)
        actions = [int(level[0, 0])] + [int(t) for t in level.ravel()] + [int(a) for a in arng.integers(0, 7, extra["edits"])]
    else:
        actions = [int(a) for a in arng.integers(0, rules.num_actions, steps)]
    T = len(actions)

    def ref_state():
        r = u._rep.unwrapped
        return np.array(r._map, dtype=np.uint8), [int(r._pos[0]), int(r._pos[1])], [int(u._rep_stats[k]) for k in R.STAT_KEYS]

    def note_search():
        rec = rules.rec
        if rec["it2"] == 0 and rec["won"]:
            seen.setdefault("win in pass 1", []).append(name)
        elif rec["won"] or (rec["it1"] == power and rec["it2"] == power):
            seen.setdefault("win in pass 2 only or both passes on the cap", []).append(name)

    ob, _ = env.reset()
    ob = np.asarray(ob).astype(np.uint8)
    r_ob = rules.reset()
    note_search()
    m, pos, st = ref_state()
    assert ob.shape == r_ob.shape and (ob == r_ob).all() and (m == rules.grid).all() and pos == rules.pos and st == rules.stats
    out = {k: [] for k in ("pos", "stats", "reward", "done", "iteration", "changes", "obs_crc")}
    full = {"steps": [-1], "map": [m], "obs": [ob]}
    pos0, stats0, obs0_crc = pos, st, crc(ob)
    after_end = False
    for t, a in enumerate(actions):
        searches = rules.searches
        ob, rew, done, trunc, info = env.step(a)
        assert done == trunc
        ob = np.asarray(ob).astype(np.uint8)
        st = [int(u._rep_stats[k]) for k in R.STAT_KEYS]
        it, ch = int(u._iteration), int(u._changes)
        assert (info["iterations"], info["changes"]) == (it, ch)
        r_ob, r_rew, r_done, r_info = rules.step(a, auto_reset=True)
        assert ("dist-floor" in info) == r_info["changed"], (name, t)
        if done:
            ob, _ = env.reset()
            ob = np.asarray(ob).astype(np.uint8)
            seen.setdefault("automatic reset", []).append(name)
            seen.setdefault("done by changes" if (cp is not None and ch > u._max_changes) else "done by iterations", []).append(name)
            note_search()
        elif r_info["searched"]:
            note_search()
        if r_info["changed"] and not r_info["searched"]:
            seen.setdefault("edit that kept solidity", []).append(name)
        if not r_info["changed"] and (rep == "narrow" or a >= 4):
            seen.setdefault("no-change step", []).append(name)
        assert rules.searches - searches == int(r_info["searched"]) + int(done)
        m, pos, _ = ref_state()
        # the rules reproduce every recorded field
        assert (ob == r_ob).all() and (m == rules.grid).all() and pos == rules.pos, (name, t)
        assert st == (r_info["final_stats"] if done else r_info["stats"]), (name, t, st, r_info)
        assert float(rew) == r_rew and bool(done) == r_done and (it, ch) == (r_info["iteration"], r_info["changes"]), (name, t)
        for k, v in (("pos", pos), ("stats", st), ("reward", float(rew)), ("done", int(done)), ("iteration", it), ("changes", ch),
                     ("obs_crc", crc(ob))):
            out[k].append(v)
        if t == 0 or t == T - 1 or after_end:
            full["steps"].append(t)
            full["map"].append(m)
            full["obs"].append(ob)
        after_end = bool(done)
        if "paint" in extra and t == h * w:  # the painted map is the level, and it wins
            assert (m == level).all() and rules.rec["won"], name
    arrays = {
        "representation": np.asarray(rep), "map_shape": np.asarray(shape, np.int32), "obs_window": np.asarray(rules.window, np.int32),
        "seed": np.int64(seed), "solver_power": np.int32(power), "max_board_scans": np.int32(3),
        "change_percentage": np.float64(-1.0 if cp is None else cp), "max_iterations": np.int32(rules.max_iterations),
        "max_changes": np.int32(-1 if rules.max_changes is None else rules.max_changes),
        "weights": np.asarray([float(weights[k]) for k in R.STAT_KEYS]), "stat_keys": np.asarray(R.STAT_KEYS),
        "actions": np.asarray(actions, np.int32), "pos": np.asarray(out["pos"], np.int32),
        "stats": np.asarray(out["stats"], np.int32), "reward": np.asarray(out["reward"], np.float64),
        "done": np.asarray(out["done"], np.uint8), "iteration": np.asarray(out["iteration"], np.int32),
        "changes": np.asarray(out["changes"], np.int32), "obs_crc": np.asarray(out["obs_crc"], np.uint32),
        "pos0": np.asarray(pos0, np.int32), "stats0": np.asarray(stats0, np.int32), "obs0_crc": np.uint32(obs0_crc),
        "full_steps": np.asarray(full["steps"], np.int32), "full_map": np.stack(full["map"]).astype(np.uint8),
        "full_obs": np.stack(full["obs"]).astype(np.uint8),
    }
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    return os.path.getsize(path), int(np.sum(out["done"])), rules.searches


def main():
    assert ref_env.available(), "the reference tree is needed"
    os.makedirs(OUT, exist_ok=True)
    seen, total = {}, 0
    for name, (rep, shape, seed, steps, power, extra) in EPISODES.items():
        size, ends, searches = record(name, rep, shape, seed, steps, power, extra, seen)
        assert size <= 100 * 1024, (name, size)
        total += size
        print(f"{name}: {size} bytes, {ends} episode ends, {searches} searches", flush=True)
    assert total <= 400 * 1024, total
    for c in CASES:
        assert seen.get(c), f"no episode shows: {c}"
        print(f"{c}: {len(seen[c])} times, e.g. {seen[c][0]}")
    print(total, "bytes in all")


if __name__ == "__main__":
    main()
