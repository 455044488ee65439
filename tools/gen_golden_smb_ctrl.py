"""Controllable Super Mario Bros episodes, recorded from the REFERENCE on the CPU (through oracle/ref_env.py, unchanged) ->
tests/golden/smb_ctrl/*.npz.  Data only; needs the reference tree; about a minute on one core.  Not for the GPU machine.

    python tools/gen_golden_smb_ctrl.py

One file per run (EPISODES): make_env(cfg) of the reference for smb with cfg.controls set (cfg.evaluate keeps make_env from adding
UniformNoiseyTargets, which cannot be constructed at this commit), seeded once, solver_power 300.  Targets are queued with
set_trgs() at the steps `events` lists; when a step ends an episode the env is reset (its streams continue) and the step's
observation and control values are the new episode's first, as SmbVecEnv reports them with auto_reset.  Arrays, T = steps:
  representation, map_shape [2], seed, solver_power, change_percentage (-1 = none), weights [9], stat_keys, controls [K]
  events       a JSON string: [[t, {metric: value | [lo, hi]}], ...]: set_trgs before step t is taken (-1: before the first reset)
  dyadic       uint8 [T]: the step's reward is a sum of multiples of 0.25 -- bit-equal in every order of the sum
  actions int32 [T], stats int32 [T][9] (of the finished episode where one ended), reward float64 [T], done uint8 [T],
  ctrl float64 [T][2K] (asserted constant over their planes), obs_crc uint32 [T] (zlib.crc32 of the uint8 map part [oh][ow][8]),
  stats0, ctrl0, obs0_crc   the same after the first reset
  reset_at int32 [R] (-1, then the steps that ended an episode), reset_lo / reset_hi float64 [R][9] and reset_shown float64
  [R][K]: the targets in force after that reset (the zero-loss intervals, and what the control observation shows)

The script fails unless tests/smb_ctrl_rules.py reproduces every recorded field -- statistics and control values exactly, rewards
bit for bit where `dyadic` and within 1e-9 elsewhere (the reference sums its loss terms in Python-set order) -- and unless the
set shows each case of CASES.
"""
import json
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
import smb_ctrl_rules as CR  # noqa: E402
import ref_env  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "smb_ctrl")
POWER = 300
ALL9 = list(R.STAT_KEYS)
CASES = ["non-integer reward", "controlled metric crosses its target", "reset with nothing queued", "queued tuple",
         "done by iterations", "done by changes", "re-queue before the reset"]


def uniform(controls, seed):
    g = np.random.default_rng(seed)
    return {k: float(g.random() * (CR.COND_BOUNDS[k][1] - CR.COND_BOUNDS[k][0]) + CR.COND_BOUNDS[k][0]) for k in controls}


# name: representation, (H, W), seed, controls, whole episodes (or "paint"), extras, events as (episode, offset, trgs):
# set_trgs `offset` steps into `episode` (episode -1: before the first reset)
EPISODES = {
    "narrow_4x5_jumps_sol": ("narrow", (4, 5), 31, ["jumps", "sol-length"], 3, {}, [
        (0, 5, {"jumps": 77.0}),  # replaced by the next one before any reset
        (0, 30, uniform(["jumps", "sol-length"], 1)),
        (1, 10, {"jumps": 3.25, "sol-length": 11.75})]),
    "turtle_5x7_cp02_tuple": ("turtle", (5, 7), 32, ["enemies", "empty", "dist-win"], 3, {"change_percentage": 0.2}, [
        (0, 2, {"enemies": (2, 5), "empty": 17.5}),
        (1, 1, {"dist-win": 3.25})]),
    "paint_8x20_sol": ("narrow", (8, 20), 33, ["sol-length"], "paint", {"paint": ("structured", 0), "edits": 20}, [
        (-1, 0, {"sol-length": 12.5})]),
    "narrow_4x5_all9": ("narrow", (4, 5), 34, ALL9, 2, {}, [
        (-1, 0, uniform(ALL9, 2)),
        (0, 7, {k: float(v) for k, v in zip(ALL9, (1.5, 0.25, 2.0, 12.75, 3.5, 1.25, 2.5, 4.0, 6.5))})]),
}


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes()) & 0xFFFFFFFF


def is_dyadic(trg):
    return all(float(4 * x).is_integer() for v in trg.values() for x in v)


def record(name, rep, shape, seed, controls, episodes, extra, plan, seen):
    h, w = shape
    K = len(controls)
    weights = dict(R.DEFAULT_WEIGHTS)
    cp = extra.get("change_percentage")
    cfg = ref_env.make_cfg("smb", rep, shape, weights=dict(weights), change_percentage=cp)
    cfg.controls = list(controls)
    cfg.evaluate = True
    env = ref_env.make_reference_env(cfg, seed=seed)
    u = env.unwrapped
    assert type(u._prob).__name__ == "SMBCtrlProblem"
    u._prob._solver_power = POWER
    rules = CR.SmbCtrlRules(rep, shape, controls, seed=seed, weights=weights, change_percentage=cp, solver_power=POWER)
    assert env.observation_space.shape == (2 * h, 2 * w, 8 + 2 * K)
    assert {k: env.param_ranges[k] for k in controls} == rules.ranges
    arng = np.random.default_rng(1000 + seed)
    paint = None
    if episodes == "paint":
        level = sl.make(extra["paint"][0], extra["paint"][1], h, w)
        paint = [int(level[0, 0])] + [int(t) for t in level.ravel()] + [int(a) for a in arng.integers(0, 7, extra["edits"])]

    def split(ob):
        o = np.asarray(ob)
        c = o[0, 0, :2 * K].astype(np.float64).copy()
        assert np.all(o[..., :2 * K] == c), "control planes must be constant"
        return c, o[..., 2 * K:].astype(np.uint8)

    def queue(trgs):
        env.set_trgs(dict(trgs))
        rules.set_trgs(dict(trgs))
        if any(isinstance(v, tuple) for v in trgs.values()):
            seen.setdefault("queued tuple", []).append(name)

    events, pending = [], 0
    for ep, off, trgs in plan:
        if ep == -1:
            queue(trgs)
            events.append([-1, {k: list(v) if isinstance(v, tuple) else v for k, v in trgs.items()}])
            pending += 1
    ob, _ = env.reset()
    r_ob = rules.reset()
    c, m = split(ob)
    st = [int(u._rep_stats[k]) for k in R.STAT_KEYS]
    assert (m == r_ob).all() and st == rules.stats and c.tolist() == rules.ctrl_obs(), name
    if pending == 0:
        seen.setdefault("reset with nothing queued", []).append(name)
    out = {k: [] for k in ("actions", "stats", "reward", "done", "ctrl", "obs_crc", "dyadic")}
    resets = {"at": [-1], "lo": [[rules.trg[k][0] for k in R.STAT_KEYS]], "hi": [[rules.trg[k][1] for k in R.STAT_KEYS]],
              "shown": [[rules.shown[k] for k in controls]]}
    stats0, ctrl0, obs0_crc = st, c, crc(m)
    episode, in_ep, t, pending = 0, 0, 0, 0
    side = {k: None for k in controls}
    while True:
        for ep, off, trgs in plan:
            if ep == episode and off == in_ep:
                if pending:
                    seen.setdefault("re-queue before the reset", []).append(name)
                queue(trgs)
                events.append([t, {k: list(v) if isinstance(v, tuple) else v for k, v in trgs.items()}])
                pending += 1
        a = paint[t] if paint is not None else int(arng.integers(0, rules.num_actions))
        dy = is_dyadic(rules.trg)
        ob, rew, done, trunc, info = env.step(a)
        st = [int(u._rep_stats[k]) for k in R.STAT_KEYS]
        for k in controls:  # a controlled metric passes from one side of its target to the other inside an episode
            v, (lo, hi) = st[R.STAT_KEYS.index(k)], rules.trg[k]
            s = -1 if v < lo else (1 if v > hi else 0)
            if side[k] is not None and s != 0 and side[k] != 0 and s != side[k]:
                seen.setdefault("controlled metric crosses its target", []).append(name)
            side[k] = s if s != 0 else side[k]
        r_ob, r_rew, r_done, r_info = rules.step(a, auto_reset=True)
        if done:
            ch = int(u._changes)
            seen.setdefault("done by changes" if (cp is not None and ch > u._max_changes) else "done by iterations", []).append(name)
            ob, _ = env.reset()
            if pending == 0:
                seen.setdefault("reset with nothing queued", []).append(name)
            pending = 0
            side = {k: None for k in controls}
            resets["at"].append(t)
            resets["lo"].append([rules.trg[k][0] for k in R.STAT_KEYS])
            resets["hi"].append([rules.trg[k][1] for k in R.STAT_KEYS])
            resets["shown"].append([rules.shown[k] for k in controls])
            for k in R.STAT_KEYS:  # the reference's targets in force are the rules'
                assert CR.interval(env.metric_trgs[k]) == rules.trg[k], (name, t, k)
        c, m = split(ob)
        # the rules reproduce every recorded field
        assert (m == r_ob).all() and bool(done) == r_done, (name, t)
        assert st == (r_info["final_stats"] if done else r_info["stats"]), (name, t)
        assert c.tolist() == rules.ctrl_obs(), (name, t, c.tolist(), rules.ctrl_obs())
        rew = float(rew)
        assert (rew == r_rew) if dy else (abs(rew - r_rew) <= 1e-9), (name, t, rew, r_rew)
        if rew != int(rew):
            seen.setdefault("non-integer reward", []).append(name)
        for k, v in (("actions", a), ("stats", st), ("reward", rew), ("done", int(done)), ("ctrl", c), ("obs_crc", crc(m)),
                     ("dyadic", int(dy))):
            out[k].append(v)
        t += 1
        in_ep += 1
        if done:
            episode, in_ep = episode + 1, 0
        if (paint is not None and t == len(paint)) or (paint is None and episode == episodes):
            break
    arrays = {
        "representation": np.asarray(rep), "map_shape": np.asarray(shape, np.int32), "seed": np.int64(seed),
        "solver_power": np.int32(POWER), "change_percentage": np.float64(-1.0 if cp is None else cp),
        "weights": np.asarray([float(weights[k]) for k in R.STAT_KEYS]), "stat_keys": np.asarray(R.STAT_KEYS),
        "controls": np.asarray(controls), "events": np.asarray(json.dumps(events)),
        "dyadic": np.asarray(out["dyadic"], np.uint8), "actions": np.asarray(out["actions"], np.int32),
        "stats": np.asarray(out["stats"], np.int32), "reward": np.asarray(out["reward"], np.float64),
        "done": np.asarray(out["done"], np.uint8), "ctrl": np.asarray(out["ctrl"], np.float64),
        "obs_crc": np.asarray(out["obs_crc"], np.uint32), "stats0": np.asarray(stats0, np.int32),
        "ctrl0": np.asarray(ctrl0, np.float64), "obs0_crc": np.uint32(obs0_crc),
        "reset_at": np.asarray(resets["at"], np.int32), "reset_lo": np.asarray(resets["lo"], np.float64),
        "reset_hi": np.asarray(resets["hi"], np.float64), "reset_shown": np.asarray(resets["shown"], np.float64),
    }
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    return os.path.getsize(path), t, int(np.sum(out["done"])), int(np.sum(out["dyadic"]))


def main():
    assert ref_env.available(), "the reference tree is needed"
    os.makedirs(OUT, exist_ok=True)
    seen, total = {}, 0
    for name, (rep, shape, seed, controls, episodes, extra, plan) in EPISODES.items():
        size, steps, ends, dyadic = record(name, rep, shape, seed, controls, episodes, extra, plan, seen)
        assert size <= 16 * 1024, (name, size)
        total += size
        print(f"{name}: {size} bytes, {steps} steps, {ends} episode ends, {dyadic} dyadic steps", flush=True)
    for c in CASES:
        assert seen.get(c), f"no episode shows: {c}"
        print(f"{c}: {len(seen[c])} times, e.g. {seen[c][0]}")
    print(total, "bytes in all")


if __name__ == "__main__":
    main()
