"""GPU: minecraft_3D_maze under the turtle and wide representations.
  (a) every reference episode of tests/golden/reps3d/ replayed from the seed alone: grid, position, statistics, reward, done,
      counters and the observation of EVERY step (crop + one-hot of the reference's obs["map"] for turtle, its one-hot for wide);
  (b) lockstep at batch size against a model built here: the representation update in numpy, statistics from the CPU oracle's
      stats_for_grids on the grid read back with get_state, the loss from the weights and targets; the path overlay against a
      3-D NARROW engine (oracle-checked code) reset to the grid of each env's last statistics update;
  (c) every other entry point against single steps.
Bars: everything bit-exact; |reward - expected| <= 1e-6 (float32 output of integer values), as the narrow 3-D replay."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import pcgrl_oracle as po  # noqa: E402  (checker only)
from conftest import GOLDEN  # noqa: E402

PROBLEM = "minecraft_3D_maze"
REPS3D = os.path.join(GOLDEN, "reps3d")
FIXTURES = sorted(glob.glob(os.path.join(REPS3D, "*.npz")))
REPLAY = [p for p in FIXTURES if not os.path.basename(p).startswith("control3d_")]
CONTROL = [p for p in FIXTURES if os.path.basename(p).startswith("control3d_")]
REW_TOL = 1e-6
REPS = ["turtle", "wide"]


def _vec(*a, **k):
    from control_pcgrl_amd import VecPcgrlEnv
    return VecPcgrlEnv(*a, **k)


def _n_actions(rep, shape):
    return 6 if rep == "turtle" else int(np.prod(shape)) * 2


def expected_obs(rep, shape, overlay_map, pos):
    """the engine's observation from the reference's obs["map"] (0 AIR, 1 DIRT, 2 path) and position"""
    m = np.asarray(overlay_map).reshape(shape).astype(np.int64)
    if rep == "wide":
        return np.eye(3, dtype=np.uint8)[m]
    ow = tuple(2 * s for s in shape)
    padded = np.pad(m + 1, [(w // 2, w // 2) for w in ow], constant_values=0)
    sl = tuple(slice(int(p), int(p) + w) for p, w in zip(pos, ow))
    return np.eye(4, dtype=np.uint8)[padded[sl]]


# ------------------------------------------------------------------------------------------------ (a) golden replay
@pytest.mark.parametrize("path", REPLAY, ids=[os.path.basename(p)[:-4] for p in REPLAY])
def test_golden_replay(path):
    z = np.load(path)
    rep, shape = str(z["representation"]), tuple(int(s) for s in z["map_shape"])
    kw = {"change_percentage": float(z["change_percentage"])} if "change_percentage" in z.files else {}
    env = _vec(PROBLEM, rep, shape, 1, seeds=[int(z["seed"])], auto_reset=False, **kw)
    assert env.num_actions == int(z["n_actions"]) == _n_actions(rep, shape)
    assert env.obs_shape == (shape + (3,) if rep == "wide" else tuple(2 * s for s in shape) + (4,))
    T = len(z["action"])
    resets = {int(s): k for k, s in enumerate(z["reset_step"])}

    def check_reset(k):
        obs, _ = env.reset()
        st = env.get_state()
        assert np.array_equal(st.grids[0].cpu().numpy().ravel(), z["reset_grid"][k]), "reset grid (RNG stream)"
        if rep == "turtle":  # (wide: the reference keeps a stale position across resets; it is not part of the observation)
            assert np.array_equal(st.pos[0].cpu().numpy(), z["reset_pos"][k]), "reset position (RNG stream)"
        assert np.array_equal(st.stats[0].cpu().numpy(), z["reset_stats"][k])
        assert np.array_equal(obs[0].cpu().numpy(), expected_obs(rep, shape, z["reset_obs"][k], z["reset_pos"][k])), "reset obs"

    check_reset(0)
    acts = torch.as_tensor(z["action"], dtype=torch.int32, device=env.device)
    for t in range(T):
        obs, rew, done, _, info = env.step(acts[t:t + 1])
        st = env.get_state()
        assert np.array_equal(st.grids[0].cpu().numpy().ravel(), z["grid"][t]), f"grid @ {t}"
        assert np.array_equal(st.pos[0].cpu().numpy(), z["pos"][t]), f"pos @ {t}"
        got = info["stats"][0].cpu().numpy()
        assert np.array_equal(got, z["stats"][t]), f"stats @ {t}: {got} vs {z['stats'][t]}"
        assert abs(float(rew[0]) - z["reward"][t]) <= REW_TOL, f"reward @ {t}"
        assert bool(done[0]) == bool(z["done"][t]), f"done @ {t}"
        assert int(st.changes[0]) == z["changes"][t] and int(st.iteration[0]) == z["iterations"][t], f"counters @ {t}"
        assert np.array_equal(obs[0].cpu().numpy(), expected_obs(rep, shape, z["overlay"][t], z["pos"][t])), f"obs/overlay @ {t}"
        if t + 1 in resets and t + 1 < T:
            check_reset(resets[t + 1])
    env.check_errors()


@pytest.mark.parametrize("path", CONTROL, ids=[os.path.basename(p)[:-4] for p in CONTROL])
def test_golden_control_replay(path):
    """control targets (n_jump, path-length) set through queue_targets: the reference's rewards for float targets and the
    control observation by its formula, next to everything the plain replay checks"""
    z = np.load(path)
    rep, shape = str(z["representation"]), tuple(int(s) for s in z["map_shape"])
    controls = [str(c) for c in z["controls"]]
    env = _vec(PROBLEM, rep, shape, 1, seeds=[int(z["seed"])], auto_reset=False, controls=controls, reward_dtype=torch.float64)
    n, t = int(z["steps_per_episode"]), 0
    acts = torch.as_tensor(z["action"], dtype=torch.int32, device=env.device)
    for ep in range(len(z["reset_at"])):
        env.queue_targets({k: float(v) for k, v in zip(controls, z["reset_trg"][ep])})
        obs, info = env.reset()
        st = env.get_state()
        assert np.array_equal(st.grids[0].cpu().numpy().ravel(), z["reset_grid"][ep])
        assert np.array_equal(st.stats[0].cpu().numpy(), z["reset_stats"][ep])
        assert np.allclose(info["ctrl_obs"][0].cpu().numpy(), z["reset_ctrl"][ep], rtol=1e-6, atol=1e-7)
        for _ in range(n):
            obs, rew, done, _, info = env.step(acts[t:t + 1])
            assert np.array_equal(info["stats"][0].cpu().numpy(), z["stats"][t]), f"stats @ {t}"
            assert abs(float(rew[0]) - z["reward"][t]) <= 1e-9, f"reward @ {t}"
            assert np.allclose(info["ctrl_obs"][0].cpu().numpy(), z["ctrl"][t], rtol=1e-6, atol=1e-7), f"ctrl @ {t}"
            assert np.array_equal(obs[0].cpu().numpy(), expected_obs(rep, shape, z["overlay"][t], z["pos"][t])), f"obs @ {t}"
            t += 1
    env.check_errors()


# ------------------------------------------------------------------------------------------------ (b) the model
class Model:
    """PcgrlEnv.step (pcgrl_env.py:267-342) over turtle_rep.update_pos / wide_rep.update for N envs in numpy.  Statistics come
    from the CPU oracle on whatever grid it is handed; an auto-reset takes the new map and position from the engine (the
    generator is pinned by the golden replays) and recomputes everything else."""

    def __init__(self, rep, shape, n, change_percentage=None):
        from control_pcgrl_amd.problems import problem_spec, target_interval
        self.rep, self.shape, self.n = rep, tuple(shape), n
        self.n_cells = int(np.prod(shape))
        self.max_iterations = self.n_cells * 3 + 1
        self.max_changes = None if change_percentage is None else max(int(change_percentage * self.n_cells), 1)
        spec = problem_spec(PROBLEM, shape)
        self.w = np.array([float(spec.default_weights.get(k, 0.0)) for k in spec.stat_keys])
        iv = [target_interval(spec.static_trgs[k]) for k in spec.stat_keys]
        self.lo, self.hi = np.array([a for a, _ in iv]), np.array([b for _, b in iv])

    def stats_of(self, grids):
        return po.stats_for_grids(PROBLEM, np.ascontiguousarray(grids.reshape((-1,) + self.shape)), threads=8).astype(np.int64)

    def loss(self, stats):  # control_wrappers.py:318-345: -sum w * distance to the target interval
        s = stats.astype(np.float64)
        d = np.where(s < self.lo, self.lo - s, np.where(s > self.hi, s - self.hi, 0.0))
        return -(d * self.w).sum(axis=1)

    def load(self, state, rows=None):
        """(re)start rows from the engine's state after a reset"""
        g = state.grids.cpu().numpy().reshape(self.n, -1)
        p = state.pos.cpu().numpy().astype(np.int64)
        if rows is None:
            rows = np.ones(self.n, bool)
            self.grid, self.pos = g.copy(), p.copy()
            self.stats = np.zeros((self.n, 3), np.int64)
            self.iteration, self.changes = np.zeros(self.n, np.int64), np.zeros(self.n, np.int64)
            self.upd_grid = g.copy()
        self.grid[rows], self.pos[rows] = g[rows], p[rows]
        self.stats[rows] = self.stats_of(self.grid[rows])
        self.iteration[rows] = 0
        self.changes[rows] = 0
        self.upd_grid[rows] = self.grid[rows]  # (a reset computes the statistics, and with them the path the next steps show)
        self.last_loss = self.loss(self.stats)

    def update(self, a):
        """the representation update alone; returns `change` per env.  self.shown_*: what the observation of this step shows"""
        a = np.asarray(a, np.int64)
        d0, d1, d2 = self.shape
        rows = np.arange(self.n)
        self.shown_upd_grid = self.upd_grid.copy()
        self.shown_fresh = np.zeros(self.n, bool)  # rows whose observation is the first of an episode: no overlay
        if self.rep == "turtle":
            mv = a < 4
            step = np.where(a & 1, 1, -1)
            ax0, ax1 = mv & (a < 2), mv & (a >= 2)
            self.pos[ax0, 0] = np.clip(self.pos[ax0, 0] + step[ax0], 0, d0 - 1)
            self.pos[ax1, 1] = np.clip(self.pos[ax1, 1] + step[ax1], 0, d1 - 1)  # the third coordinate never moves
            cell = (self.pos[:, 0] * d1 + self.pos[:, 1]) * d2 + self.pos[:, 2]
            tile = np.where(mv, self.grid[rows, cell], a - 4)
        else:
            cell, tile = a >> 1, a & 1
            self.pos = np.stack(np.unravel_index(cell, self.shape), axis=1).astype(np.int64)
        change = self.grid[rows, cell] != tile
        self.grid[rows, cell] = tile
        return change

    def step(self, a, engine_grids):
        """one PcgrlEnv.step; `engine_grids`: the maps read back from the engine after its step, compared and -- for the
        statistics -- used where the episode goes on (an env that auto-reset already holds its next map)"""
        change = self.update(a)
        self.iteration += 1
        self.changes += change
        done = self.iteration > self.max_iterations
        if self.max_changes is not None:
            done = done | (self.changes > self.max_changes)
        assert np.array_equal(engine_grids[~done], self.grid[~done]), "grid"
        if change.any():
            src = np.where(done[:, None], self.grid, engine_grids)
            self.stats[change] = self.stats_of(src[change])
            self.upd_grid[change] = self.grid[change]
        loss = self.loss(self.stats)
        rew, self.last_loss = loss - self.last_loss, loss
        return rew, done


def _overlay_maps(shape, grids):
    """the path tiles the observation shows after a statistics update on `grids`, from a 3-D NARROW engine: reset to the
    grids, one step that changes nothing (it re-writes cell 0), and the overlay channel of its (whole-map) window"""
    n = len(grids)
    nar = _vec(PROBLEM, "narrow", shape, n, auto_reset=False)
    g = torch.as_tensor(np.ascontiguousarray(grids.reshape((n,) + tuple(shape))))
    nar.reset(init_grids=g)
    obs, *_ = nar.step(torch.as_tensor(grids[:, 0].astype(np.int32)).to(nar.device))
    pos = nar.get_state().pos.cpu().numpy()
    assert (pos == pos[0]).all()
    o = obs.cpu().numpy()
    sl = tuple(slice(int(s - p), int(2 * s - p)) for s, p in zip(shape, pos[0]))
    win = o[(slice(None),) + sl]
    assert (win[..., 0] == 0).all()  # the whole map is inside the window
    nar.check_errors()
    nar.close()
    return win[..., 3].reshape(n, -1).astype(bool)


def _check_obs(model, rep, obs, paths=None, rows=None):
    """the observation against the model: off the path everywhere; the path tiles where `paths` (from _overlay_maps) are given"""
    shape, n = model.shape, model.n
    o = obs.cpu().numpy()
    codes = o.argmax(-1)
    assert (o.sum(-1) == 1).all(), "one-hot"
    if rep == "wide":
        m = codes.reshape(n, -1)
    else:  # un-crop: map cell i sits at window index i + dims - pos
        m = np.empty((n, model.n_cells), np.int64)
        for e in range(n):
            sl = tuple(slice(int(s - p), int(2 * s - p)) for s, p in zip(shape, model.pos[e]))
            w = codes[e][sl]
            full = np.ones(codes[e].shape, bool)
            full[sl] = False
            assert (codes[e][full] == 0).all() and (w > 0).all(), "out-of-bounds channel"
            m[e] = w.ravel() - 1
    path = m == 2
    assert np.array_equal(m[~path], model.grid[~path]), "tiles off the path"
    assert not path[model.shown_fresh].any(), "the first observation of an episode carries no overlay"
    if paths is not None:
        sel = ~model.shown_fresh if rows is None else rows
        assert np.array_equal(path[sel], paths[sel]), "path overlay"


def _lockstep(rep, shape, n, T, change_percentage, overlay_every, seed):
    env = _vec(PROBLEM, rep, shape, n, seeds=seed + np.arange(n), auto_reset=True, change_percentage=change_percentage)
    model = Model(rep, shape, n, change_percentage)
    obs, _ = env.reset()
    model.load(env.get_state())
    assert np.array_equal(env.get_state().stats.cpu().numpy(), model.stats)
    g = torch.Generator().manual_seed(seed)
    n_resets = 0
    for t in range(T):
        a = torch.randint(0, env.num_actions, (n,), generator=g, dtype=torch.int32)
        obs, rew, done, _, info = env.step(a.to(env.device))
        st = env.get_state()
        eg = st.grids.cpu().numpy().reshape(n, -1)
        d_eng = done.cpu().numpy().astype(bool)
        wrew, wdone = model.step(a.numpy(), eg)
        assert np.array_equal(d_eng, wdone), f"done @ {t}"
        assert np.array_equal(info["stats"].cpu().numpy(), model.stats), f"stats @ {t}"
        assert np.max(np.abs(rew.cpu().numpy().astype(np.float64) - wrew)) <= REW_TOL, f"reward @ {t}"
        cont = ~wdone
        assert np.array_equal(st.pos.cpu().numpy()[cont], model.pos[cont]), f"pos @ {t}"
        assert np.array_equal(st.iteration.cpu().numpy()[cont], model.iteration[cont]) and \
            np.array_equal(st.changes.cpu().numpy()[cont], model.changes[cont]), f"counters @ {t}"
        if wdone.any():  # auto-reset: new map and position from the engine, statistics and counters re-derived
            n_resets += int(wdone.sum())
            model.load(st, wdone)
            model.shown_fresh = wdone.copy()
            assert np.array_equal(st.stats.cpu().numpy()[wdone], model.stats[wdone]), f"reset stats @ {t}"
            assert (st.iteration.cpu().numpy()[wdone] == 0).all() and (st.changes.cpu().numpy()[wdone] == 0).all()
            if rep == "turtle":
                p = st.pos.cpu().numpy()[wdone]
                assert (p >= 0).all() and (p < np.array(shape)).all()
        paths = None
        if overlay_every and (t % overlay_every == overlay_every - 1 or t == T - 1):
            paths = _overlay_maps(shape, model.shown_upd_grid)
        _check_obs(model, rep, obs, paths)
    model.shown_fresh[:] = True  # pcgrl_observe: the map and position as they are, no overlay (what reset() hands out)
    _check_obs(model, rep, env.observe())
    env.check_errors()
    return n_resets


@pytest.mark.parametrize("rep", REPS)
def test_lockstep_1024_envs_7cubed(rep):
    """1024 envs, every env, every step; change_percentage makes episodes end (and auto-reset) inside the run"""
    resets = _lockstep(rep, (7, 7, 7), 1024, 420, 0.1 if rep == "turtle" else 0.3, 60, 11)
    assert resets > 512


@pytest.mark.parametrize("rep", REPS)
def test_lockstep_15cubed(rep):
    resets = _lockstep(rep, (15, 15, 15), 48, 160, 0.004 if rep == "turtle" else 0.012, 40, 5)
    assert resets > 24


@pytest.mark.parametrize("rep,shape", [("turtle", (5, 6, 7)), ("wide", (5, 6, 7)), ("wide", (4, 3, 5)), ("turtle", (10, 10, 10))])
def test_lockstep_other_shapes(rep, shape):
    """the run-time-dimension kernels of both size classes (wide rows of 630 and 180 bytes)"""
    _lockstep(rep, shape, 64, 150, 0.2, 50, 3)


# ------------------------------------------------------------------------------------------------ (c) other entry points
def _actions(rep, shape, K, n, seed):
    return torch.randint(0, _n_actions(rep, shape), (K, n), dtype=torch.int32, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("rep", REPS)
def test_rollout_equals_single_steps(rep):
    n, K, shape, kw = 96, 260, (7, 7, 7), dict(change_percentage=0.15)
    seeds = 3 + np.arange(n)
    a = _actions(rep, shape, K, n, 9)
    ref = _vec(PROBLEM, rep, shape, n, seeds=seeds, auto_reset=True, **kw)
    ref.reset()
    want = []
    for t in range(K):
        obs, rew, done, _, info = ref.step(a[t].to(ref.device))
        want.append((obs.clone(), rew.clone(), done.clone(), info["stats"].clone()))
    assert torch.stack([w[2] for w in want]).any()  # episodes ended and auto-reset inside the run
    for form in ("all", "last", "none"):
        env = _vec(PROBLEM, rep, shape, n, seeds=seeds, auto_reset=True, **kw)
        env.reset()
        parts = [env.rollout(a[lo:hi].to(env.device), want_obs=form) for lo, hi in [(0, 3), (3, K)]]
        rew, done, stats = (torch.cat([p[i] for p in parts]) for i in (1, 2, 3))
        for t in range(K):
            assert torch.equal(stats[t], want[t][3]) and torch.equal(rew[t], want[t][1]), f"{form} @ {t}"
            assert torch.equal(done[t].bool(), want[t][2].bool()), f"{form} done @ {t}"
        if form == "all":
            obs_all = torch.cat([p[0] for p in parts])
            for t in range(K):
                assert torch.equal(obs_all[t], want[t][0]), f"obs @ {t}"
        elif form == "last":
            assert torch.equal(parts[-1][0], want[-1][0])
        sa, sb = env.get_state(), ref.get_state()
        assert torch.equal(sa.grids, sb.grids) and torch.equal(sa.pos, sb.pos) and torch.equal(sa.stats, sb.stats)
        env.check_errors()
    a15 = _actions(rep, (15, 15, 15), 40, 8, 2)  # size class 1
    e1, e2 = (_vec(PROBLEM, rep, (15, 15, 15), 8, seeds=np.arange(8), auto_reset=True, change_percentage=0.002) for _ in range(2))
    e1.reset(); e2.reset()
    obs_all, rew, done, stats = e1.rollout(a15.to(e1.device), want_obs="all")
    for t in range(40):
        obs, r, d, _, info = e2.step(a15[t].to(e2.device))
        assert torch.equal(obs_all[t], obs) and torch.equal(stats[t], info["stats"]) and torch.equal(rew[t], r), f"15^3 @ {t}"
    assert done.any()


@pytest.mark.parametrize("rep", REPS)
def test_update_and_refresh_stats_equal_steps(rep):
    """rep.update() K times without PcgrlEnv.step(), get_stats() once, then steps: maps, positions and statistics are those of
    an env that stepped through the same actions; the counters stay untouched"""
    n, shape = 128, (7, 7, 7)
    seeds = 5 + np.arange(n)
    a = _actions(rep, shape, 90, n, 3)
    env = _vec(PROBLEM, rep, shape, n, seeds=seeds, auto_reset=False)
    ref = _vec(PROBLEM, rep, shape, n, seeds=seeds, auto_reset=False)
    model = Model(rep, shape, n)
    env.reset(); ref.reset()
    model.load(env.get_state())
    reset_paths = _overlay_maps(shape, model.upd_grid)
    for t in range(50):
        obs = env.update(a[t].to(env.device))
        ref.step(a[t].to(ref.device))
        model.update(a[t].numpy())
        # nothing updated the statistics since the reset: the overlay stays the reset's path
        _check_obs(model, rep, obs, reset_paths if t % 10 == 9 else None)
    sa, sb = env.get_state(), ref.get_state()
    assert torch.equal(sa.grids, sb.grids) and torch.equal(sa.pos, sb.pos)
    assert int(sa.iteration.max()) == 0 and int(sa.changes.max()) == 0
    assert torch.equal(env.refresh_stats(), sb.stats)
    for t in range(50, 60):
        o1, r1, d1, _, i1 = env.step(a[t].to(env.device))
        o2, r2, d2, _, i2 = ref.step(a[t].to(ref.device))
        assert torch.equal(i1["stats"], i2["stats"]) and torch.equal(o1, o2) and torch.equal(r1, r2), f"@ {t}"
    # a step right after updates WITHOUT a refresh: statistics are recomputed from scratch where the step changes the map
    for t in range(60, 66):
        env.update(a[t].to(env.device), want_obs=False)
    g0 = env.get_state().grids.clone()
    _, _, _, _, info = env.step(a[70].to(env.device))
    g1 = env.get_state().grids
    changed = (g0 != g1).reshape(n, -1).any(1)
    assert changed.any()
    want = torch.as_tensor(model.stats_of(g1.cpu().numpy().reshape(n, -1)), device=env.device)
    assert torch.equal(info["stats"][changed].long(), want[changed])
    assert torch.equal(env.refresh_stats().long(), want)
    env.check_errors()


@pytest.mark.parametrize("rep", REPS)
def test_checkpoint_round_trip_mid_episode(rep):
    n, shape = 64, (7, 7, 7)
    a = _actions(rep, shape, 120, n, 4)
    src = _vec(PROBLEM, rep, shape, n, seeds=np.arange(n), auto_reset=True, change_percentage=0.2)
    src.reset()
    for t in range(60):
        src.step(a[t].to(src.device))
    sd = src.state_dict()
    dst = _vec(PROBLEM, rep, shape, n, seeds=900 + np.arange(n), auto_reset=True, change_percentage=0.2)
    dst.load_state_dict(sd)
    for t in range(60, 120):
        o1, r1, d1, _, i1 = src.step(a[t].to(src.device))
        o2, r2, d2, _, i2 = dst.step(a[t].to(dst.device))
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(i1["stats"], i2["stats"]), t
    # an image of another representation is refused, not reinterpreted
    other = _vec(PROBLEM, "narrow" if rep == "wide" else "wide", shape, n, seeds=np.arange(n))
    with pytest.raises((ValueError, RuntimeError, NotImplementedError)):
        other.load_state_dict(sd)
    nar = _vec(PROBLEM, "narrow", shape, n, seeds=np.arange(n))
    nar.reset()
    with pytest.raises((ValueError, RuntimeError, NotImplementedError)):
        dst.load_state_dict(nar.state_dict())


@pytest.mark.parametrize("rep", REPS)
def test_step_loop_in_a_hip_graph(rep):
    n, shape = 128, (7, 7, 7)
    seeds = 40 + np.arange(n)
    env = _vec(PROBLEM, rep, shape, n, seeds=seeds, auto_reset=True, change_percentage=0.2)
    ref = _vec(PROBLEM, rep, shape, n, seeds=seeds, auto_reset=True, change_percentage=0.2)
    env.reset(); ref.reset()
    a = _actions(rep, shape, 203, n, 6)
    static_a = torch.zeros(n, dtype=torch.int32, device=env.device)
    for t in range(3):  # (eager warm-up before the capture)
        env.step(a[t].to(env.device)); ref.step(a[t].to(ref.device))
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            obs, rew, done, _, info = env.step(static_a)
    torch.cuda.current_stream().wait_stream(side)
    for t in range(3, 203):
        static_a.copy_(a[t])
        graph.replay()
        o2, r2, d2, _, i2 = ref.step(a[t].to(ref.device))
        assert torch.equal(info["stats"], i2["stats"]) and torch.equal(rew, r2) and torch.equal(done, d2), f"@ {t}"
        assert torch.equal(obs, o2), f"obs @ {t}"
    env.check_errors()


@pytest.mark.parametrize("rep", REPS)
@pytest.mark.parametrize("shape", [(7, 7, 7), (5, 6, 7)])
def test_codes_form(rep, shape):
    from control_pcgrl_amd import codes_to_onehot
    n = 64
    seeds = 7 + np.arange(n)
    env = _vec(PROBLEM, rep, shape, n, seeds=seeds, obs_format="codes")
    ref = _vec(PROBLEM, rep, shape, n, seeds=seeds)
    assert env.obs_shape == ref.obs_shape[:-1] + (1,)
    oc, _ = env.reset()
    oo, _ = ref.reset()
    assert torch.equal(codes_to_onehot(oc, env), oo)
    a = _actions(rep, shape, 80, n, 1)
    for t in range(80):
        oc, r1, d1, _, i1 = env.step(a[t].to(env.device))
        oo, r2, d2, _, i2 = ref.step(a[t].to(ref.device))
        assert torch.equal(codes_to_onehot(oc, env), oo), f"@ {t}"
        assert int(oc.max()) <= (2 if rep == "wide" else 3)
        assert torch.equal(i1["stats"], i2["stats"]) and torch.equal(r1, r2)
    assert torch.equal(codes_to_onehot(env.observe(), env), ref.observe())
    oc_all = env.rollout(a[:5].to(env.device), want_obs="all")[0]
    oo_all = ref.rollout(a[:5].to(ref.device), want_obs="all")[0]
    assert torch.equal(codes_to_onehot(oc_all, env), oo_all)
    env.check_errors()


@pytest.mark.parametrize("rep", REPS)
def test_sub_batched_env_equals_one_batch(rep):
    from control_pcgrl_amd import make_vec_env
    n, k, shape = 96, 3, (7, 7, 7)
    cfg = {"task": {"problem": PROBLEM, "map_shape": list(shape), "obs_window": None, "weights": None}, "representation": rep,
           "change_percentage": 0.2}
    env = make_vec_env(cfg, n, seeds=700 + np.arange(n), sub_batches=k)
    ref = make_vec_env(cfg, n, seeds=700 + np.arange(n))
    assert env.k == k and env.num_actions == _n_actions(rep, shape)
    o1, _ = env.reset()
    o2, _ = ref.reset()
    assert torch.equal(o1, o2)
    a = _actions(rep, shape, 100, n, 5)
    for t in range(100):
        o1, r1, d1, _, i1 = env.step(a[t].to(ref.device))
        o2, r2, d2, _, i2 = ref.step(a[t].to(ref.device))
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1.bool(), d2.bool()) and torch.equal(i1["stats"], i2["stats"]), t
    env.check_errors()


@pytest.mark.parametrize("rep", REPS)
def test_adapters_against_golden(rep):
    """make_env (gym call shape) and PcgrlVectorEnv (three reference episodes side by side in one engine)"""
    from control_pcgrl_amd import PcgrlVectorEnv, flatten_wide_action, make_env
    zs = [np.load(os.path.join(REPS3D, f"episode_mc3dmaze_{rep}_s{s}.npz")) for s in (1, 2, 3)]
    shape = tuple(int(s) for s in zs[0]["map_shape"])
    cfg = {"task": {"problem": PROBLEM, "map_shape": list(shape), "obs_window": None, "weights": None}, "representation": rep}
    venv = PcgrlVectorEnv(cfg, num_envs=3, seeds=[int(z["seed"]) for z in zs], obs_dtype=np.float32)
    assert venv.action_space.n == _n_actions(rep, shape)
    assert venv.observation_space.shape == (shape + (3,) if rep == "wide" else tuple(2 * s for s in shape) + (4,))
    obs, _ = venv.vector_reset()
    for k, z in enumerate(zs):
        assert np.array_equal(obs[k].astype(np.uint8), expected_obs(rep, shape, z["reset_obs"][0], z["reset_pos"][0]))
    for t in range(150):
        obs, rew, term, trunc, infos = venv.vector_step([int(z["action"][t]) for z in zs])
        for k, z in enumerate(zs):
            assert np.array_equal(obs[k].astype(np.uint8), expected_obs(rep, shape, z["overlay"][t], z["pos"][t])), f"env {k} @ {t}"
            assert abs(rew[k] - z["reward"][t]) <= REW_TOL and term[k] == bool(z["done"][t])
    z = zs[0]
    env = make_env(cfg)
    env.seed(int(z["seed"]))
    assert env.action_space.n == _n_actions(rep, shape) and env.observation_space.shape == venv.observation_space.shape
    out = env.reset()
    obs = out[0] if isinstance(out, tuple) else out
    assert np.array_equal(np.asarray(obs).astype(np.uint8), expected_obs(rep, shape, z["reset_obs"][0], z["reset_pos"][0]))
    for t in range(150):
        act = int(z["action"][t])
        if rep == "wide":  # the reference's MultiDiscrete action, flattened
            multi = np.unravel_index(act, shape + (2,))
            assert int(flatten_wide_action(multi, shape, 2)) == act
        obs, rew, done, *rest = env.step(act)
        info = rest[-1]
        assert np.array_equal(np.asarray(obs).astype(np.uint8), expected_obs(rep, shape, z["overlay"][t], z["pos"][t])), t
        assert abs(rew - z["reward"][t]) <= REW_TOL and bool(done) == bool(z["done"][t])
        assert [info[str(k)] for k in z["stat_keys"]] == z["stats"][t].tolist()


@pytest.mark.parametrize("rep", REPS)
def test_sampler_and_bad_actions(rep):
    """pcgrl_sample_actions draws from the whole action space; an action outside it sets the error bit (poll_error raises)
    and changes nothing"""
    n, shape = 256, (7, 7, 7)
    env = _vec(PROBLEM, rep, shape, n, seeds=np.arange(n), auto_reset=False)
    env.reset()
    na = _n_actions(rep, shape)
    assert env.num_actions == na
    seen = torch.cat([env.sample_actions(seed=s).clone() for s in range(40)])
    assert int(seen.min()) >= 0 and int(seen.max()) < na
    distinct = len(torch.unique(seen))  # 10 240 uniform draws: all 6 turtle actions, and nearly all of wide's 686
    assert distinct == 6 if rep == "turtle" else distinct > 600
    env.step(seen[:n].to(env.device))
    env.check_errors()
    before = env.get_state()
    bad = torch.full((n,), na, dtype=torch.int32)
    bad[1::2] = -1
    env.step(bad.to(env.device))
    with pytest.raises(ValueError):
        env.check_errors()
    after = env.get_state()
    assert torch.equal(before.grids, after.grids) and torch.equal(before.pos, after.pos) and torch.equal(before.stats, after.stats)


@pytest.mark.parametrize("rep", REPS)
def test_reset_with_injected_maps_and_target_resampling(rep):
    """pcgrl_reset(init_grids[, init_pos]) and device-side target resampling in controllable mode"""
    n, shape = 64, (7, 7, 7)
    z = np.load(os.path.join(GOLDEN, "stats_mc3dmaze.npz"))
    grids = torch.as_tensor(z["grids"][-n:])
    pos = torch.as_tensor(np.stack([np.arange(n) % 7, (np.arange(n) // 7) % 7, (np.arange(n) * 3) % 7], 1).astype(np.int32))
    env = _vec(PROBLEM, rep, shape, n, seeds=np.arange(n), auto_reset=False)
    obs, _ = env.reset(init_grids=grids, init_pos=pos)
    st = env.get_state()
    assert torch.equal(st.grids.cpu(), grids) and np.array_equal(st.stats.cpu().numpy(), z["stats"][-n:])
    if rep == "turtle":
        assert torch.equal(st.pos.cpu(), pos)
    model = Model(rep, shape, n)
    model.load(st)
    model.shown_fresh = np.ones(n, bool)
    _check_obs(model, rep, obs)
    env.check_errors()
    ctl = _vec(PROBLEM, rep, shape, n, seeds=np.arange(n), auto_reset=True, controls=["n_jump", "path-length"],
               change_percentage=0.03)  # 10 changes end an episode (a turtle changes the map every sixth step or so)
    ctl.set_target_resampling(True, seed=5)
    ctl.reset()
    c0 = ctl.ctrl_obs.clone()
    a = _actions(rep, shape, 200, n, 8)
    dones = 0
    for t in range(200):
        _, _, d, _, info = ctl.step(a[t].to(ctl.device))
        dones += int(d.sum())
    c1 = info["ctrl_obs"]
    assert dones > 0 and not torch.equal(c0[:, 0::2], c1[:, 0::2])  # targets were redrawn at the auto-resets
    ctl.check_errors()
