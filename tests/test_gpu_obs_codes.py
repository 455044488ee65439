"""The tile-code observation form (obs_format="codes", include/pcgrl_amd_codes.h) on the GPU: the reference's golden
episodes in code form, lockstep against a one-hot twin (same seeds and actions: codes_to_onehot(codes) == onehot bit for
bit, same reward / done / stats), rollouts in every form, asynchronous stepping, graph capture, sub-batching, checkpoints,
the CPU oracle and the RLlib adapter."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pcgrl_oracle as po  # noqa: E402  (checker only)
from conftest import GOLDEN  # noqa: E402


def _vec(*a, **k):
    from control_pcgrl_amd import VecPcgrlEnv
    return VecPcgrlEnv(*a, **k)


def _to_onehot(codes, env):
    from control_pcgrl_amd import codes_to_onehot
    return codes_to_onehot(codes, env)


def _twins(problem, rep, shape, n, **kw):
    seeds = 11 + np.arange(n)
    a = _vec(problem, rep, shape, n, seeds=seeds, **kw)
    b = _vec(problem, rep, shape, n, seeds=seeds, obs_format="codes", **kw)
    assert b.obs_format == "codes" and b.onehot_shape == a.obs_shape
    return a, b


def _same_obs(codes, onehot, env, what):
    got = _to_onehot(codes, env)
    if not torch.equal(got, onehot):
        bad = (got != onehot).reshape(onehot.shape[0], -1).any(1).nonzero().flatten()
        raise AssertionError(f"{what}: codes != one-hot in {bad.numel()} envs, first {bad[:5].tolist()}")


def _random_actions(env, g):
    shape = (env.num_envs, env.action_entries) if env.action_entries > 1 else (env.num_envs,)
    hi = env.spec.n_tiles if env.action_entries > 1 else env.num_actions
    return torch.randint(0, hi, shape, generator=g, dtype=torch.int32).to(env.device)


def _lockstep(problem, rep, shape, n, min_episodes=2, max_steps=3000, **kw):
    """auto-reset twins until every env has finished `min_episodes` episodes (maps above 16 x 16 take a change_percentage:
    by default an episode lasts 3 board scans)"""
    a, b = _twins(problem, rep, shape, n, **kw)
    oa, _ = a.reset()
    ob, _ = b.reset()
    _same_obs(ob, oa, b, "reset")
    g = torch.Generator().manual_seed(5)
    episodes = torch.zeros(n, dtype=torch.int64, device=a.device)
    t = 0
    while t < max_steps:
        act = _random_actions(a, g)
        oa, ra, da, _, ia = a.step(act)
        ob, rb, db, _, ib = b.step(act)
        _same_obs(ob, oa, b, f"step {t}")
        assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ia["stats"], ib["stats"]), f"step {t}"
        if "ctrl_obs" in ia:
            assert torch.equal(ia["ctrl_obs"], ib["ctrl_obs"]), f"ctrl_obs @ {t}"
        episodes += da.long()
        t += 1
        if t % 64 == 0 and int(episodes.min()) >= min_episodes:
            break
    assert int(episodes.min()) >= min_episodes, f"only {int(episodes.min())} episodes in {t} steps"
    a.check_errors()
    b.check_errors()
    return a, b


# ------------------------------------------------------------------------------------------------ golden episodes
EPISODES = sorted(glob.glob(os.path.join(GOLDEN, "episode_*.npz")))


@pytest.mark.parametrize("path", EPISODES, ids=[os.path.basename(p)[8:-4] for p in EPISODES])
def test_golden_episode_in_codes(path):
    """the reference's recorded episodes replayed in code form: at every recorded observation the codes are the argmax of
    the reference's one-hot image (3-D: the overlay map + 1, padded and cropped around pos)"""
    z = np.load(path)
    problem, rep = str(z["problem"]), str(z["representation"])
    shape = tuple(int(s) for s in z["map_shape"])
    env = _vec(problem, rep, shape, 1, seeds=[int(z["seed"])], auto_reset=False, obs_format="codes")
    T, ep_len = len(z["action"]), int(z["episode_len"])
    three_d = len(shape) == 3

    def want_2d(flat):
        return np.asarray(flat).reshape(tuple(int(s) for s in z["obs_shape"])).argmax(-1)

    def want_3d(overlay_map, pos):
        m = overlay_map.reshape(shape).astype(np.int64) + 1
        ow = tuple(2 * s for s in shape)
        padded = np.pad(m, [(w // 2, w // 2) for w in ow], constant_values=0)
        return padded[tuple(slice(int(p), int(p) + w) for p, w in zip(pos, ow))]

    def check_reset(k):
        obs, _ = env.reset()
        o = obs[0, ..., 0].cpu().numpy()
        want = want_3d(z["reset_obs"][k], z["reset_pos"][k]) if three_d else want_2d(z["reset_obs"][k])
        assert np.array_equal(o, want), f"reset {k}"

    check_reset(0)
    obs_steps = {} if three_d else {int(s): i for i, s in enumerate(z["obs_steps"])}
    acts = torch.as_tensor(z["action"], dtype=torch.int32, device=env.device)
    for t in range(T):
        obs, rew, done, _, info = env.step(acts[t:t + 1])
        assert np.array_equal(info["stats"][0].cpu().numpy(), z["stats"][t]), f"stats @ {t}"
        if three_d:
            assert np.array_equal(obs[0, ..., 0].cpu().numpy(), want_3d(z["overlay"][t], z["pos"][t])), f"obs @ {t}"
        elif t in obs_steps:
            assert np.array_equal(obs[0, ..., 0].cpu().numpy(), want_2d(z["obs_full"][obs_steps[t]])), f"obs @ {t}"
        if t == ep_len - 1:
            check_reset(1)
    env.check_errors()


# ------------------------------------------------------------------------------------------------ lockstep with a twin
@pytest.mark.parametrize("problem,rep,shape,n,kw", [
    ("binary", "narrow", (16, 16), 4096, {}),
    ("zelda", "turtle", (16, 16), 4096, {}),
    ("sokoban", "wide", (16, 16), 2048, {}),
    ("binary", "narrow", (32, 32), 256, {"change_percentage": 0.1}),
    ("binary", "narrow", (64, 64), 64, {"change_percentage": 0.05}),
    ("zelda", "narrow", (16, 16), 512, {"static_prob": 0.1, "n_static_walls": 3}),
    ("binary", "narrow", (16, 16), 512, {"act_window": (3, 3)}),
    ("binary", "narrow", (16, 16), 512, {"controls": ["regions", "path-length"], "reward_dtype": torch.float64}),
    ("zelda", "narrow", (16, 16), 512, {"obs_window": (15, 9)}),
    ("binary", "turtle", (16, 16), 512, {"obs_window": (3, 3)}),
    ("zelda", "narrow", (16, 16), 256, {"obs_window": (15, 9), "static_prob": 0.2}),
    ("sokoban", "narrow", (20, 20), 256, {"change_percentage": 0.1}),
    ("binary", "wide", (8, 8), 256, {}),
], ids=["binary-narrow", "zelda-turtle", "sokoban-wide", "binary32", "binary64", "zelda-static", "binary-aw3x3", "binary-ctrl",
        "zelda-15x9", "binary-3x3", "zelda-15x9-static", "sokoban20", "binary-wide8"])
def test_lockstep_2d(problem, rep, shape, n, kw):
    _lockstep(problem, rep, shape, n, **kw)


def test_lockstep_maze_7():
    _lockstep("minecraft_3D_maze", "narrow", (7, 7, 7), 1024, max_steps=2500)


def test_lockstep_maze_15():
    _lockstep("minecraft_3D_maze", "narrow", (15, 15, 15), 32, change_percentage=0.02)


def test_observe_and_update_in_codes():
    a, b = _twins("zelda", "narrow", (16, 16), 256, obs_window=(9, 15))
    a.reset()
    b.reset()
    g = torch.Generator().manual_seed(2)
    for t in range(30):
        act = _random_actions(a, g)
        _same_obs(b.update(act), a.update(act), b, f"update {t}")
    assert torch.equal(a.refresh_stats(), b.refresh_stats())
    _same_obs(b.observe(), a.observe(), b, "observe")


# ------------------------------------------------------------------------------------------------ rollouts
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("want", ["all", "last", "none"])
def test_rollout_forms_in_codes(form, want):
    from control_pcgrl_amd import _lib
    a, b = _twins("binary", "narrow", (16, 16), 512)
    for e in (a, b):
        _lib.check(e._L.pcgrl_set_rollout_form(e._h, form), "pcgrl_set_rollout_form")
        e.reset()
    g = torch.Generator().manual_seed(9)
    for _ in range(3):
        acts = torch.randint(0, a.num_actions, (24, a.num_envs), generator=g, dtype=torch.int32).cuda()
        oa, ra, da, sa = a.rollout(acts, want_obs=want)
        ob, rb, db, sb = b.rollout(acts, want_obs=want)
        assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(sa, sb)
        if want == "none":
            assert oa is None and ob is None
        else:
            _same_obs(ob, oa, b, f"rollout {want}")
    _same_obs(b.observe(), a.observe(), b, "after rollouts")


@pytest.mark.parametrize("problem,rep,kw", [("zelda", "turtle", {}), ("zelda", "narrow", {"controls": ["regions"],
                                                                                           "reward_dtype": torch.float64})])
def test_rollout_all_per_step_encoder(problem, rep, kw):
    """zelda (9 bytes per cell): rollout(want_obs="all") in codes form as K x (step + encoder)"""
    a, b = _twins(problem, rep, (16, 16), 512, **kw)
    a.reset()
    b.reset()
    g = torch.Generator().manual_seed(12)
    for _ in range(3):
        acts = torch.randint(0, a.num_actions, (40, a.num_envs), generator=g, dtype=torch.int32).cuda()
        oa, ra, da, sa = a.rollout(acts, want_obs="all")
        ob, rb, db, sb = b.rollout(acts, want_obs="all")
        assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(sa, sb)
        _same_obs(ob, oa, b, "rollout all")
        if a.ctrl_obs is not None:
            assert torch.equal(a.ctrl_obs, b.ctrl_obs)
    _same_obs(b.observe(), a.observe(), b, "after rollouts")


def test_rollout_all_in_codes_3d_and_chunks(monkeypatch):
    from control_pcgrl_amd import vec_env
    a, b = _twins("minecraft_3D_maze", "narrow", (7, 7, 7), 64)
    a.reset()
    b.reset()
    monkeypatch.setattr(vec_env, "_ROLLOUT_SCRATCH_BYTES", 3 * 64 * int(np.prod(a.obs_shape)))  # chunks of 3 steps
    g = torch.Generator().manual_seed(4)
    acts = torch.randint(0, a.num_actions, (20, a.num_envs), generator=g, dtype=torch.int32).cuda()
    oa, ra, da, sa = a.rollout(acts, want_obs="all")
    ob, rb, db, sb = b.rollout(acts, want_obs="all")
    assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(sa, sb)
    _same_obs(ob, oa, b, "3-D rollout all")
    acts = torch.randint(0, a.num_actions, (7, a.num_envs), generator=g, dtype=torch.int32).cuda()
    _same_obs(b.rollout(acts, want_obs="last")[0], a.rollout(acts, want_obs="last")[0], b, "3-D rollout last")


# ------------------------------------------------------------------------------------------------ asynchronous stepping
def test_step_ready_in_codes():
    """sokoban with a solver budget (the 6 x 6 setting of the asynchronous-stepping tests: random maps are playable often
    enough that searches get parked): every row, busy envs' included, is the code form of the twin's one-hot row"""
    n, steps = 256, 300
    kw = dict(change_percentage=0.2, solver_power=400)
    seeds = 1000 + np.arange(n)
    a = _vec("sokoban", "wide", (6, 6), n, seeds=seeds, **kw)
    b = _vec("sokoban", "wide", (6, 6), n, seeds=seeds, obs_format="codes", **kw)
    for e in (a, b):
        e.set_solver_budget(12)
    oa, _ = a.reset()
    ob, _ = b.reset()
    _same_obs(ob, oa, b, "reset")
    rng = np.random.default_rng(3)
    tiles = rng.choice(5, size=(steps, n), p=[0.5, 0.1, 0.1, 0.15, 0.15])
    acts = torch.as_tensor((rng.integers(0, 36, size=(steps, n)) * 5 + tiles).astype(np.int32)).cuda()
    busy_seen = 0
    for t in range(steps):
        oa, ra, da, _, ia = a.step_ready(acts[t])
        ob, rb, db, _, ib = b.step_ready(acts[t])
        assert torch.equal(ia["status"], ib["status"]), f"status @ {t}"
        emitted = (ia["status"] & 1).bool()
        busy_seen += int((~emitted).sum())
        assert torch.equal(ra[emitted], rb[emitted]) and torch.equal(da[emitted], db[emitted])
        assert torch.equal(ia["stats"][emitted], ib["stats"][emitted])
        _same_obs(ob, oa, b, f"step_ready {t}")
    assert busy_seen > 0, "no env was ever busy: the test did not exercise parked searches"
    a.check_errors()
    b.check_errors()


# ------------------------------------------------------------------------------------------------ graphs, sub-batches, checkpoints
def test_graph_capture_of_codes_steps():
    n = 1024
    eager = _vec("zelda", "turtle", (16, 16), n, seeds=np.arange(n), obs_format="codes")
    graphed = _vec("zelda", "turtle", (16, 16), n, seeds=np.arange(n), obs_format="codes")
    eager.reset()
    graphed.reset()
    g = torch.Generator().manual_seed(3)
    acts = torch.randint(0, eager.num_actions, (20, n), generator=g, dtype=torch.int32).cuda()
    obs_hist = torch.empty((20,) + tuple(graphed._obs.shape), dtype=torch.uint8, device="cuda")
    rew_hist = torch.empty((20, n), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for k in range(20):
                o, r, _, _, _ = graphed.step(acts[k])
                obs_hist[k].copy_(o)
                rew_hist[k].copy_(r)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    for k in range(20):
        o, r, _, _, _ = eager.step(acts[k])
        assert torch.equal(o, obs_hist[k]) and torch.equal(r, rew_hist[k]), f"graph step {k}"
    torch.cuda.synchronize()


def test_sub_batched_codes():
    from control_pcgrl_amd import SubBatchedVecEnv
    n = 512
    one = _vec("binary", "narrow", (32, 32), n, seeds=np.arange(n), obs_format="codes")
    sub = SubBatchedVecEnv("binary", "narrow", (32, 32), n, sub_batches=2, seeds=np.arange(n), obs_format="codes")
    assert sub.obs_shape == one.obs_shape == (64, 64, 1)
    assert torch.equal(sub.reset()[0], one.reset()[0])
    g = torch.Generator().manual_seed(6)
    for t in range(60):
        act = _random_actions(one, g)
        os_, rs, ds, _, is_ = sub.step(act)
        oo, ro, do, _, io = one.step(act)
        assert torch.equal(os_, oo) and torch.equal(rs, ro) and torch.equal(is_["stats"], io["stats"]), f"step {t}"
    assert torch.equal(sub.observe(), one.observe())


def test_checkpoint_from_onehot_into_codes():
    n = 256
    src = _vec("zelda", "turtle", (16, 16), n, seeds=np.arange(n))
    src.reset()
    g = torch.Generator().manual_seed(8)
    for _ in range(25):
        src.step(_random_actions(src, g))
    sd = src.state_dict()
    dst = _vec("zelda", "turtle", (16, 16), n, seeds=np.arange(n) + 999, obs_format="codes")
    dst.load_state_dict(sd)
    _same_obs(dst.observe(), src.observe(), dst, "after load")
    for t in range(120):
        act = _random_actions(src, g)
        oa, ra, da, _, ia = src.step(act)
        ob, rb, db, _, ib = dst.step(act)
        _same_obs(ob, oa, dst, f"step {t}")
        assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ia["stats"], ib["stats"])


# ------------------------------------------------------------------------------------------------ oracle, RLlib adapter
@pytest.mark.parametrize("problem,rep,shape", [("binary", "narrow", (16, 16)), ("zelda", "turtle", (16, 16)),
                                               ("sokoban", "wide", (16, 16)), ("minecraft_3D_maze", "narrow", (7, 7, 7))])
def test_codes_against_oracle(problem, rep, shape):
    n = 256
    seeds = 7 + np.arange(n)
    env = _vec(problem, rep, shape, n, seeds=seeds, obs_format="codes")
    orc = po.OracleVecEnv(problem, rep, shape, n, seeds=seeds)
    obs, _ = env.reset()
    assert np.array_equal(obs[..., 0].cpu().numpy(), orc.reset().argmax(-1))
    g = torch.Generator().manual_seed(0)
    for t in range(60):
        a = torch.randint(0, env.num_actions, (n,), generator=g, dtype=torch.int32)
        obs, rew, done, _, info = env.step(a.cuda())
        oobs, orew, odone, ostats = orc.step(a.numpy(), auto_reset=True)
        assert np.array_equal(info["stats"].cpu().numpy(), ostats), t
        assert np.array_equal(obs[..., 0].cpu().numpy(), oobs.argmax(-1)), f"obs @ {t}"
    env.check_errors()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_rllib_adapter_codes(dtype):
    from control_pcgrl_amd import PcgrlVectorEnv
    n = 512
    cfg = {"task": {"problem": "binary", "map_shape": (16, 16)}, "representation": "narrow"}
    a = PcgrlVectorEnv(cfg, num_envs=n, seeds=np.arange(n), obs_dtype=dtype)
    b = PcgrlVectorEnv(dict(cfg, obs_format="codes"), num_envs=n, seeds=np.arange(n), obs_dtype=dtype)
    sp = b.observation_space
    assert sp.shape == (32, 32, 1) and np.dtype(sp.dtype) == np.dtype(dtype) and float(np.max(sp.high)) == 2.0

    def check(oa, ob, what):
        ob = np.stack(ob)
        assert ob.dtype == np.dtype(dtype) and ob.shape[1:] == sp.shape
        assert (ob >= sp.low).all() and (ob <= sp.high).all(), what
        assert np.array_equal(np.eye(3, dtype=np.float64)[ob[..., 0].astype(np.int64)], np.stack(oa).astype(np.float64)), what

    check(a.vector_reset()[0], b.vector_reset()[0], "reset")
    rng = np.random.default_rng(2)
    for t in range(150):
        act = rng.integers(0, 2, n)
        oa, ra, da, _, _ = a.vector_step(act)
        ob, rb, db, _, _ = b.vector_step(act)
        check(oa, ob, f"step {t}")
        assert ra == rb and da == db
        for i in [i for i, d in enumerate(da) if d]:
            check([a.reset_at(i)[0]], [b.reset_at(i)[0]], f"reset_at {i}")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ more entry points
def test_nontemporal_stores_in_codes(monkeypatch):
    """the encoder's non-temporal branch (the one-hot kernels' rule: observation bytes per launch >= PCGRL_OBS_NT_MB,
    read at pcgrl_create; 1 MB here so that 4096 16 x 16 envs -- 4 MB of codes -- take it)"""
    monkeypatch.setenv("PCGRL_OBS_NT_MB", "1")
    _lockstep("zelda", "turtle", (16, 16), 4096, min_episodes=1)
    _lockstep("binary", "narrow", (32, 32), 1024, min_episodes=1, change_percentage=0.1)


def test_gym_env_codes():
    from control_pcgrl_amd import make_env
    cfg = {"task": {"problem": "zelda", "map_shape": (16, 16)}, "representation": "narrow", "static_prob": 0.1}
    a = make_env(cfg)
    b = make_env(dict(cfg, obs_format="codes"))
    sp = b.observation_space
    assert sp.shape == (32, 32, 2) and float(sp.high[..., 0].max()) == 8.0 and float(sp.high[..., 1].max()) == 1.0
    a.seed(3)
    b.seed(3)

    def same(oa, ob, what):
        assert ob.dtype == np.float32 and ob.shape == sp.shape and (ob >= sp.low).all() and (ob <= sp.high).all(), what
        oh = np.concatenate((np.eye(9, dtype=np.float32)[ob[..., 0].astype(np.int64)], ob[..., 1:]), -1)
        assert np.array_equal(oh, oa), what

    same(a.reset()[0], b.reset()[0], "reset")
    rng = np.random.default_rng(1)
    for t in range(60):
        act = int(rng.integers(0, 8))
        oa, ra, da, _, ia = a.step(act)
        ob, rb, db, _, ib = b.step(act)
        same(oa, ob, f"step {t}")
        assert ra == rb and da == db and ia == ib
        if da:
            same(a.reset()[0], b.reset()[0], f"reset @ {t}")


def test_rllib_adapter_codes_with_controls():
    """control planes (float32, in front) + codes"""
    from control_pcgrl_amd import PcgrlVectorEnv
    n = 256
    cfg = {"task": {"problem": "binary", "map_shape": (16, 16)}, "representation": "narrow", "controls": ["regions", "path-length"]}
    a = PcgrlVectorEnv(cfg, num_envs=n, seeds=np.arange(n))
    b = PcgrlVectorEnv(dict(cfg, obs_format="codes"), num_envs=n, seeds=np.arange(n))
    sp = b.observation_space
    assert sp.shape == (32, 32, 5) and np.array_equal(sp.high[0, 0], np.array([1, 1, 1, 1, 2], np.float32))

    def check(oa, ob, what):
        oa, ob = np.stack(oa), np.stack(ob)
        assert ob.shape[1:] == sp.shape and (ob >= sp.low).all() and (ob <= sp.high).all(), what
        assert np.array_equal(ob[..., :4], oa[..., :4]), what  # control planes
        assert np.array_equal(np.eye(3, dtype=np.float32)[ob[..., 4].astype(np.int64)], oa[..., 4:]), what

    check(a.vector_reset()[0], b.vector_reset()[0], "reset")
    rng = np.random.default_rng(4)
    for t in range(120):
        act = rng.integers(0, 2, n)
        oa, ra, da, _, _ = a.vector_step(act)
        ob, rb, db, _, _ = b.vector_step(act)
        check(oa, ob, f"step {t}")
        assert ra == rb and da == db
        for i in [i for i, d in enumerate(da) if d]:
            check([a.reset_at(i)[0]], [b.reset_at(i)[0]], f"reset_at {i}")
    a.close()
    b.close()
