"""Golden episodes of minecraft_3D_maze under the turtle and wide representations, recorded from the REFERENCE
(ControlWrapper(PcgrlEnv3D), built by oracle/ref_env.py) on the CPU -> tests/golden/reps3d/*.npz.

    python tools/gen_golden_3d_reps.py            # everything (needs the reference tree; a few minutes)

The files live in a sub-folder of tests/golden/ because the narrow replay tests collect `tests/golden/episode_mc3dmaze_*.npz`
and `shape3d_*.npz` by pattern and replay whatever matches with the narrow representation.

Layout: that of run_episode / run_shape_episode_3d / run_control_episode_3d in oracle/gen_golden.py, with the raw
obs["map"] (path overlay included) of EVERY step as `overlay`.  Actions are the engine's: turtle the reference's Discrete(6);
wide the C-order flat index over (d0, d1, d2, n_tiles), unravelled for the reference's MultiDiscrete.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import ref_env  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "reps3d")
PROBLEM = "minecraft_3D_maze"
STAT_KEYS = ["regions", "path-length", "n_jump"]
N_TILES = 2


def stats_vec(stats):
    return np.array([int(stats[k]) for k in STAT_KEYS], dtype=np.int64)


def n_actions(rep, shape):
    return 4 + N_TILES if rep == "turtle" else int(np.prod(shape)) * N_TILES


def ref_action(rep, shape, a):
    """the reference's action for the engine's int"""
    if rep == "turtle":
        return int(a)
    return np.array(np.unravel_index(int(a), tuple(shape) + (N_TILES,)), dtype=np.int64)


class Recorder:
    """steps a reference env and keeps what the replay tests compare"""

    def __init__(self, rep, shape, seed, change_percentage=None):
        self.rep, self.shape, self.seed = rep, tuple(shape), seed
        self.cfg = ref_env.make_cfg(PROBLEM, rep, shape, change_percentage=change_percentage)
        self.env = ref_env.make_reference_env(self.cfg, seed=seed)
        self.core = self.env.unwrapped
        self.rec = {k: [] for k in ("action", "grid", "pos", "stats", "reward", "done", "changes", "iterations", "overlay")}
        self.resets = {k: [] for k in ("step", "grid", "pos", "stats", "obs")}
        self.t = 0

    def grid(self):
        return self.core._rep.unwrapped._map.astype(np.uint8).copy()

    def pos(self):
        p = getattr(self.core._rep.unwrapped, "_pos", None)  # (wide: none before the first update, stale after a reset)
        return np.zeros(3, np.int64) if p is None else np.array(p, dtype=np.int64).copy()

    def reset(self):
        obs, _ = self.env.reset()
        r = self.resets
        r["step"].append(self.t); r["grid"].append(self.grid().ravel()); r["pos"].append(self.pos())
        r["stats"].append(stats_vec(self.core._rep_stats)); r["obs"].append(np.asarray(obs["map"]).astype(np.uint8).ravel().copy())

    def step(self, a):
        obs, r, d, tr, info = self.env.step(ref_action(self.rep, self.shape, a))
        assert d == tr
        c = self.rec
        c["action"].append(int(a)); c["grid"].append(self.grid().ravel()); c["pos"].append(self.pos())
        c["stats"].append(stats_vec(self.core._rep_stats)); c["reward"].append(float(r)); c["done"].append(bool(d))
        c["changes"].append(int(info["changes"])); c["iterations"].append(int(info["iterations"]))
        c["overlay"].append(np.asarray(obs["map"]).astype(np.uint8).ravel().copy())
        self.t += 1
        return bool(d)

    def save(self, name, episode_len, **extra):
        c, r = self.rec, self.resets
        out = dict(
            problem=PROBLEM, representation=self.rep, map_shape=np.array(self.shape), obs_window=np.array(self.cfg.task.obs_window),
            seed=self.seed, stat_keys=np.array(STAT_KEYS), n_actions=n_actions(self.rep, self.shape), episode_len=episode_len,
            action=np.array(c["action"], np.int32), grid=np.array(c["grid"], np.uint8),
            pos=np.array(c["pos"], np.int16), stats=np.array(c["stats"], np.int32), reward=np.array(c["reward"], np.float64),
            done=np.array(c["done"], np.bool_), changes=np.array(c["changes"], np.int32),
            iterations=np.array(c["iterations"], np.int32), overlay=np.array(c["overlay"], np.uint8),
            reset_step=np.array(r["step"], np.int32), reset_grid=np.array(r["grid"], np.uint8),
            reset_pos=np.array(r["pos"], np.int16), reset_stats=np.array(r["stats"], np.int32),
            reset_obs=np.array(r["obs"], np.uint8), **extra)
        os.makedirs(OUT, exist_ok=True)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        st = out["stats"]
        print(f"wrote {os.path.relpath(path, ROOT)}: T={self.t} ep_len={episode_len} max stats {st.max(0).tolist()} "
              f"steps with n_jump>0 {int((st[:, 2] > 0).sum())} distinct stats {len(np.unique(st, axis=0))} "
              f"reset pos {out['reset_pos'].tolist()} {os.path.getsize(path)} bytes", flush=True)
        return out


def run_to_done(R, draw, extra_steps):
    """one whole episode from a reset, its reset, and `extra_steps` of the next"""
    R.reset()
    ep_len = None
    while True:
        d = R.step(draw())
        if d:
            if ep_len is not None:
                break
            ep_len = R.t
            R.reset()
        if ep_len is not None and R.t >= ep_len + extra_steps:
            break
    return ep_len


def run_episode(rep, seed, shape=(7, 7, 7), extra_steps=24):
    R = Recorder(rep, shape, seed)
    arng = np.random.default_rng(1000 + seed)
    n = n_actions(rep, shape)
    ep_len = run_to_done(R, lambda: int(arng.integers(n)), extra_steps)
    return R.save(f"episode_mc3dmaze_{rep}_s{seed}", ep_len)


def run_shape_episode(rep, shape, max_changes, seed, extra_steps=12):
    """other map sizes (size class 1), with change_percentage so that max_changes ends the episode"""
    n_cells = int(np.prod(shape))
    cp = (max_changes + 0.5) / n_cells
    R = Recorder(rep, shape, seed, change_percentage=cp)
    assert R.core._max_changes == max_changes, (R.core._max_changes, max_changes)
    arng = np.random.default_rng(7000 + seed)
    n = n_actions(rep, shape)
    ep_len = run_to_done(R, lambda: int(arng.integers(n)), extra_steps)
    return R.save(f"shape3d_mc3dmaze_{rep}_{shape[0]}_s{seed}", ep_len, change_percentage=cp, max_changes=max_changes)


def run_control_episode(rep, seed, shape=(7, 7, 7), controls=("n_jump", "path-length"), n_steps=150):
    """control targets, set the way run_control_episode_3d of oracle/gen_golden.py sets them (ControlWrapper.set_trgs on a
    wrapper built without ctrl_metrics); the control observation by observe_metric_trgs' formula"""
    R = Recorder(rep, shape, seed)
    env, core = R.env, R.core
    arng = np.random.default_rng(2000 + seed)
    trng = np.random.default_rng(3000 + seed)
    n = n_actions(rep, shape)
    ranges = {k: abs(env.cond_bounds[k][1] - env.cond_bounds[k][0]) for k in controls}
    ctrl, reset_ctrl, reset_trg, reset_at = [], [], [], []

    def ctrl_now(trg):
        out = []
        for k, v in zip(controls, trg):
            out += [v / ranges[k], float(core._rep_stats[k]) / ranges[k]]
        return np.array(out, np.float64)

    for ep in range(2):
        trg = []
        for k in controls:
            lb, ub = env.cond_bounds[k]
            trg.append(float(trng.random() * (ub - lb) + lb))
        env.set_trgs(dict(zip(controls, trg)))
        reset_at.append(R.t)
        R.reset()
        reset_ctrl.append(ctrl_now(trg)); reset_trg.append(trg)
        for _ in range(n_steps):
            R.step(int(arng.integers(n)))
            ctrl.append(ctrl_now(trg))
    return R.save(f"control3d_mc3dmaze_{rep}_s{seed}", n_steps, controls=np.array(controls), steps_per_episode=n_steps,
                  cond_bounds=np.array([env.cond_bounds[k] for k in controls], np.float64), ctrl=np.array(ctrl, np.float64),
                  reset_at=np.array(reset_at, np.int32), reset_ctrl=np.array(reset_ctrl, np.float64),
                  reset_trg=np.array(reset_trg, np.float64))


def known_maps():
    """(stats, grid) of the committed 7^3 known-answer maps, longest paths first"""
    out = []
    for f in ("stats_mc3dmaze.npz", "stats_mc3dmaze_test3d.npz"):
        z = np.load(os.path.join(GOLDEN, f))
        for i in range(len(z["grids"])):
            if "shapes" in z.files and tuple(z["shapes"][i]) != (7, 7, 7):
                continue
            out.append((f, i, z["stats"][i].astype(np.int64), z["grids"][i].reshape(7, 7, 7).astype(np.uint8)))
    return out


def run_scripted_wide(name, seed, grid, want_stats, n_random=300, around=True):
    """writes `grid` cell by cell in C order (one cell per step), then edits randomly; asserts that the reference ends the
    scripted part on the map's known statistics"""
    shape = grid.shape
    R = Recorder("wide", shape, seed)
    R.reset()
    flat = grid.ravel()
    for cell in range(flat.size):
        R.step(cell * N_TILES + int(flat[cell]))
    got = stats_vec(R.core._rep_stats)
    assert np.array_equal(R.grid(), grid) and np.array_equal(got, want_stats), (got, want_stats)
    arng = np.random.default_rng(4000 + seed)
    for _ in range(n_random):
        R.step(int(arng.integers(n_actions("wide", shape))))
    return R.save(name, R.t, scripted_steps=flat.size, scripted_stats=np.array(want_stats, np.int32))


def run_scripted_turtle(name, seed, shape=(7, 7, 7), n_random=120):
    """the turtle carves a corridor in its slab (it can only edit cells whose third index is the one drawn at reset): it
    walks rows of axis 0 back and forth along axis 1 writing AIR on the rows it sweeps and DIRT under them, then acts randomly"""
    R = Recorder("turtle", shape, seed)
    R.reset()
    d0, d1, _ = shape
    p = R.pos()
    for _ in range(int(p[0])):  # to the corner (0, 0)
        R.step(0)
    for _ in range(int(p[1])):
        R.step(2)
    for i in range(d0):
        tile = 1 if i % 3 == 0 else 0  # floors of DIRT with two rows of AIR above them (array axis 0 is the height)
        cols = range(d1) if i % 2 == 0 else range(d1 - 1, -1, -1)
        for n, j in enumerate(cols):
            # (a floor keeps a hole at alternating ends so that the levels connect)
            hole = tile == 1 and j == (0 if (i // 3) % 2 == 0 else d1 - 1)
            R.step(4 + (0 if hole else tile))
            if n < d1 - 1:
                R.step(3 if i % 2 == 0 else 2)
        if i < d0 - 1:
            R.step(1)
    scripted = R.t
    arng = np.random.default_rng(5000 + seed)
    for _ in range(n_random):
        R.step(int(arng.integers(6)))
    return R.save(name, R.t, scripted_steps=scripted)


def pick_turtle_seeds(shape=(7, 7, 7), want=3, limit=60):
    """seeds whose reset draws the third coordinate in the interior, and one on a face (0 or d2 - 1)"""
    interior, face = [], []
    for seed in range(1, limit):
        env = ref_env.make_reference_env(ref_env.make_cfg(PROBLEM, "turtle", shape), seed=seed)
        env.reset()
        p2 = int(env.unwrapped._rep.unwrapped._pos[2])
        (face if p2 in (0, shape[2] - 1) else interior).append(seed)
        if len(interior) >= want and face:
            break
    return interior, face


def main():
    assert ref_env.available(), "the reference tree is needed to record fixtures"
    outs = {}
    for seed in (1, 2, 3):
        outs[f"turtle{seed}"] = run_episode("turtle", seed)
        outs[f"wide{seed}"] = run_episode("wide", seed, extra_steps=16)
    p2 = {k: int(v["reset_pos"][0][2]) for k, v in outs.items() if k.startswith("turtle")}
    print("third coordinate at the first reset:", p2, flush=True)
    interior, face = pick_turtle_seeds()
    print("turtle seeds: interior", interior[:6], "face", face[:3], flush=True)
    if not any(v in (0, 6) for v in p2.values()):  # one more whole episode in a boundary slab
        outs["turtle_face"] = run_episode("turtle", face[0], extra_steps=8)
    assert any(0 < v < 6 for v in p2.values())
    run_scripted_turtle("scripted_mc3dmaze_turtle_s%d" % interior[0], interior[0])
    for rep in ("turtle", "wide"):
        run_shape_episode(rep, (15, 15, 15), 30 if rep == "turtle" else 60, 81)
        run_shape_episode(rep, (10, 10, 10), 24 if rep == "turtle" else 80, 82)
        run_control_episode(rep, 11)
    # scripted wide episodes: the known maps with the longest path and with the most jumps
    maps = known_maps()
    longest = max(maps, key=lambda m: (m[2][1], m[2][2]))
    jumpy = max(maps, key=lambda m: (m[2][2], m[2][1]))
    print("longest path:", longest[:3], "most jumps:", jumpy[:3], flush=True)
    a = run_scripted_wide("scripted_mc3dmaze_wide_longest_s5", 5, longest[3], longest[2])
    b = run_scripted_wide("scripted_mc3dmaze_wide_jumps_s6", 6, jumpy[3], jumpy[2])
    # the conditions on the committed set (tests/test_3d_reps_cpu.py asserts them on the files)
    z = np.load(os.path.join(GOLDEN, "stats_mc3dmaze.npz"))
    half = (int(z["stats"][:, 1].max()) + 1) // 2
    assert max(int((a["stats"][:, 2] > 0).sum()), int((b["stats"][:, 2] > 0).sum())) > 0, "no wide fixture with n_jump > 0"
    assert max(int(a["stats"][:, 1].max()), int(b["stats"][:, 1].max())) >= half, "no wide fixture reaches half the longest path"


if __name__ == "__main__":
    main()
