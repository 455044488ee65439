"""Stepping Super Mario Bros environments on the device (SmbVecEnv, include/pcgrl_amd_smb_env.h): every fixture of
tests/golden/smb_env -- episodes recorded from the reference -- is reproduced from its seed alone, field by field and with
float64 rewards bit for bit; the kernel is compared with the plain-Python rules of tests/smb_env_rules.py on maps of its own
(which covers the two exact shortcuts through the search count); and the API's corners: batch sizes, a masked reset,
auto_reset=False, an action outside the space, a dirty workspace, a captured step replayed across an episode end."""
import os
import sys
import zlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smb_env_rules as E  # noqa: E402
import smb_levels as sl  # noqa: E402
import smb_rules as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smb_env")
FIXTURES = ["narrow_4x5", "turtle_5x7_cp02", "narrow_8x20_p300", "turtle_8x20_p300", "narrow_6x12_win5x9", "turtle_5x7_alt",
            "paint_8x30_p300", "paint_6x70_p300", "narrow_16x116", "turtle_16x116", "narrow_16x127"]
DEV = "cuda:0"


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes()) & 0xFFFFFFFF


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cp = float(z["change_percentage"])
    kw = dict(representation=str(z["representation"]), map_shape=tuple(int(s) for s in z["map_shape"]),
              obs_window=tuple(int(s) for s in z["obs_window"]), weights={k: float(w) for k, w in zip(R.STAT_KEYS, z["weights"])},
              change_percentage=None if cp < 0 else cp, solver_power=int(z["solver_power"]))
    return z, kw


def make(kw, n, seeds, **more):
    from control_pcgrl_amd import SmbVecEnv
    return SmbVecEnv(num_envs=n, device=DEV, seeds=seeds, reward_dtype=torch.float64, **kw, **more)


def replay_fixture(env, z, rows, step=None):
    """every recorded field of fixture z, on the env rows `rows` (all seeded with the fixture's seed)"""
    step = step or (lambda a: env.step(a))
    n = env.num_envs
    full = {int(t): k for k, t in enumerate(z["full_steps"])}
    obs, _ = env.reset()
    st = env.get_state()
    o = obs.cpu().numpy()
    for i in rows:
        assert crc(o[i]) == int(z["obs0_crc"]) and np.array_equal(o[i], z["full_obs"][full[-1]])
        assert st.pos[i].tolist() == list(z["pos0"]) and st.stats[i].tolist() == list(z["stats0"])
        assert np.array_equal(st.grids[i].cpu().numpy(), z["full_map"][full[-1]])
    for t, a in enumerate(z["actions"]):
        obs, rew, done, trunc, info = step(torch.full((n,), int(a), dtype=torch.int32, device=DEV))
        o, r, d, s = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), info["stats"].cpu().numpy()
        st = env.get_state()
        pos, it, ch = st.pos.cpu().numpy(), st.iteration.cpu().numpy(), st.changes.cpu().numpy()
        for i in rows:
            assert r.dtype == np.float64 and r[i] == z["reward"][t], (t, i, r[i], z["reward"][t])
            assert bool(d[i]) == bool(z["done"][t]) and bool(trunc[i]) == bool(d[i]), (t, i)
            assert s[i].tolist() == z["stats"][t].tolist(), (t, i, s[i], z["stats"][t])
            assert pos[i].tolist() == z["pos"][t].tolist(), (t, i)
            assert crc(o[i]) == int(z["obs_crc"][t]), (t, i)
            if z["done"][t]:  # the counters of the finished episode are gone: the new episode starts at 0
                assert (it[i], ch[i]) == (0, 0)
            else:
                assert (it[i], ch[i]) == (int(z["iteration"][t]), int(z["changes"][t])), (t, i)
            if t in full:
                assert np.array_equal(o[i], z["full_obs"][full[t]]), (t, i)
                assert np.array_equal(st.grids[i].cpu().numpy(), z["full_map"][full[t]]), (t, i)
    env.check_errors()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_from_the_seed_alone(name):
    z, kw = load(name)
    env = make(kw, 3, [int(z["seed"]), 999, int(z["seed"])])
    replay_fixture(env, z, (0, 2))
    ends = int(z["done"].sum())
    le = env.last_episode()
    assert le.count.tolist()[0] == ends and le.count.tolist()[2] == ends
    if ends:
        last = int(np.nonzero(z["done"])[0][-1])
        assert le.stats[0].tolist() == z["stats"][last].tolist() and int(le.length[0]) == int(z["iteration"][last])
    env.close()


@pytest.mark.parametrize("name", ["narrow_4x5", "turtle_5x7_cp02"])
def test_make_env_reproduces_the_fixture(name):
    from control_pcgrl_amd import make_env
    z, kw = load(name)
    cfg = NS(representation=kw["representation"], change_percentage=kw["change_percentage"], max_board_scans=3, controls=None,
             task=NS(problem="smb", map_shape=kw["map_shape"], obs_window=kw["obs_window"], weights=kw["weights"],
                     solver_power=kw["solver_power"]), multiagent=NS(n_agents=0))
    env = make_env(cfg, device=DEV)
    env.seed(int(z["seed"]))
    ob, info = env.reset()
    assert info == {} and ob.dtype == np.float32 and crc(ob) == int(z["obs0_crc"])
    changes = 0
    for t, a in enumerate(z["actions"]):
        ob, rew, done, trunc, info = env.step(int(a))
        assert rew == float(z["reward"][t]) and done == bool(z["done"][t]) and trunc == done, t
        assert (info["iterations"], info["changes"]) == (int(z["iteration"][t]), int(z["changes"][t])), t
        assert info["max_iterations"] == int(z["max_iterations"])
        assert info["max_changes"] == (None if int(z["max_changes"]) < 0 else int(z["max_changes"]))
        if info["changes"] != changes:  # the statistics are in info only on a step that changed the map
            assert [info[k] for k in R.STAT_KEYS] == z["stats"][t].tolist(), t
        else:
            assert "dist-floor" not in info
        changes = info["changes"]
        if done:
            ob, _ = env.reset()
            changes = 0
        assert crc(ob) == int(z["obs_crc"][t]), t
    with pytest.raises(IndexError):
        env.step(env.action_space.n)
    env.close()


def run_against_rules(env, rules, actions, auto_reset):
    """steps env and the rules of every env through actions [T][N], comparing everything each step"""
    n = env.num_envs
    for t in range(actions.shape[0]):
        obs, rew, done, _, info = env.step(torch.as_tensor(actions[t], dtype=torch.int32, device=DEV))
        o, r, d, s = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), info["stats"].cpu().numpy()
        st = env.get_state()
        pos, grids, searches = st.pos.cpu().numpy(), st.grids.cpu().numpy(), st.searches.cpu().numpy()
        last_loss = st.last_loss.cpu().numpy()
        for i in range(n):
            r_ob, r_rew, r_done, r_info = rules[i].step(int(actions[t, i]), auto_reset=auto_reset)
            ended = r_done and auto_reset
            assert s[i].tolist() == (r_info["final_stats"] if ended else r_info["stats"]), (t, i)
            assert r[i] == r_rew and bool(d[i]) == r_done, (t, i, r[i], r_rew)
            assert pos[i].tolist() == rules[i].pos and np.array_equal(grids[i], rules[i].grid), (t, i)
            assert np.array_equal(o[i], r_ob), (t, i)
            assert searches[i] == rules[i].searches and last_loss[i] == rules[i].last_loss, (t, i)
    env.check_errors()


def test_own_maps_65_envs_turtle():
    h, w, n, steps, power = 8, 30, 65, 30, 300
    rng = np.random.default_rng(5)
    grids = sl.batch(3, n, h, w)  # structured, random and walled levels
    pos = np.stack([rng.integers(0, h, n), rng.integers(0, w, n)], axis=1)
    env = make(dict(representation="turtle", map_shape=(h, w), solver_power=power), n, np.arange(n))
    rules = [E.SmbEnvRules("turtle", (h, w), seed=i, solver_power=power) for i in range(n)]
    obs, _ = env.reset(init_grids=grids, init_pos=pos)
    o = obs.cpu().numpy()
    st = env.get_state()
    for i in range(n):
        assert np.array_equal(o[i], rules[i].reset(grids[i], pos[i]))
        assert st.stats[i].tolist() == rules[i].stats and float(st.last_loss[i]) == rules[i].last_loss
    assert st.searches.tolist() == [1] * n
    # mostly writes, so that solidity-changing, solidity-keeping and no-change edits all occur in every env
    actions = np.where(rng.random((steps, n)) < 0.25, rng.integers(0, 4, (steps, n)), rng.integers(4, 11, (steps, n)))
    run_against_rules(env, rules, actions, auto_reset=True)
    total = int(env.get_state().searches.sum())
    assert n < total < n * (steps + 1)  # some edits searched, and not all of them
    env.close()


def test_own_maps_stock_size_narrow():
    h, w, n, steps = 16, 116, 4, 20
    rng = np.random.default_rng(6)
    grids = np.stack([sl.make("structured", 2, h, w), sl.make("random", 1, h, w), sl.make("walled", 0, h, w),
                      sl.make("structured", 5, h, w)])
    env = make(dict(representation="narrow", map_shape=(h, w)), n, np.arange(n))
    rules = [E.SmbEnvRules("narrow", (h, w), seed=i) for i in range(n)]
    obs, _ = env.reset(init_grids=grids)
    o = obs.cpu().numpy()
    for i in range(n):
        assert np.array_equal(o[i], rules[i].reset(grids[i]))
    assert env.get_state().stats.tolist() == [r.stats for r in rules]
    run_against_rules(env, rules, rng.integers(0, 7, (steps, n)), auto_reset=True)
    st = env.get_state()
    assert (st.search_iterations.cpu().numpy() >= st.max_search_iterations.cpu().numpy()).all()
    assert int(st.max_search_iterations.max()) <= 2 * 10000
    env.close()


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_batch_sizes_and_batch_positions(n):
    """the same seed at every batch position gives the fixture's trajectory at every one of them"""
    z, kw = load("narrow_4x5")
    env = make(kw, n, [int(z["seed"])] * n)
    obs, _ = env.reset()
    assert (obs == obs[0]).all()
    for t, a in enumerate(z["actions"][:80]):  # across the first automatic reset
        obs, rew, done, _, info = env.step(torch.full((n,), int(a), dtype=torch.int32, device=DEV))
        assert (obs == obs[0]).all() and (info["stats"] == info["stats"][0]).all()
        assert (rew == float(z["reward"][t])).all() and (done == bool(z["done"][t])).all(), t
        assert info["stats"][n - 1].tolist() == z["stats"][t].tolist() and crc(obs[n - 1].cpu().numpy()) == int(z["obs_crc"][t])
    assert z["done"][:80].sum() == 1
    env.check_errors()
    env.close()


def test_masked_reset():
    kw = dict(representation="turtle", map_shape=(5, 7))
    env = make(kw, 4, [5, 6, 7, 8])
    rules = [E.SmbEnvRules("turtle", (5, 7), seed=s) for s in (5, 6, 7, 8)]
    env.reset()
    for r in rules:
        r.reset()
    actions = np.random.default_rng(1).integers(0, 11, (6, 4))
    run_against_rules(env, rules, actions, auto_reset=True)
    before = env.get_state()
    obs, _ = env.reset(mask=[1, 0, 1, 0])
    o, st = obs.cpu().numpy(), env.get_state()
    for i in (0, 2):  # a new episode from the continuing streams
        assert np.array_equal(o[i], rules[i].reset()) and np.array_equal(st.grids[i].cpu().numpy(), rules[i].grid)
        assert (int(st.iteration[i]), int(st.changes[i])) == (0, 0) and st.stats[i].tolist() == rules[i].stats
    for i in (1, 3):  # untouched, and its observation written all the same
        assert np.array_equal(o[i], rules[i].observation()) and torch.equal(st.grids[i], before.grids[i])
        assert int(st.iteration[i]) == 6 and int(st.searches[i]) == int(before.searches[i])
    run_against_rules(env, rules, actions, auto_reset=True)
    env.close()


def test_without_auto_reset_the_episode_goes_on():
    z, kw = load("narrow_4x5")
    env = make(kw, 2, [int(z["seed"])] * 2, auto_reset=False)
    rules = [E.SmbEnvRules(seed=int(z["seed"]), shape=kw["map_shape"], **{k: v for k, v in kw.items() if k != "map_shape"})
             for _ in range(2)]
    env.reset()
    for r in rules:
        r.reset()
    actions = np.repeat(z["actions"][:66, None], 2, axis=1)
    run_against_rules(env, rules, actions, auto_reset=False)
    st = env.get_state()
    assert st.iteration.tolist() == [66, 66] and st.searches.tolist() == [rules[0].searches] * 2
    assert env.last_episode().count.tolist() == [5, 5]  # done at every step from iteration 62 on, latched each time
    env.close()


def test_action_outside_the_space():
    kw = dict(representation="narrow", map_shape=(4, 5))
    env = make(kw, 3, [1, 2, 3])
    obs0 = env.reset()[0].clone()
    before = env.get_state()
    obs, rew, done, _, info = env.step(torch.tensor([1, 7, -1], dtype=torch.int32, device=DEV))
    st = env.get_state()
    assert st.iteration.tolist() == [1, 0, 0] and rew[1:].tolist() == [0.0, 0.0] and done.tolist() == [False] * 3
    assert torch.equal(obs[1:], obs0[1:]) and torch.equal(st.grids[1:], before.grids[1:])
    assert torch.equal(info["stats"][1:], before.stats[1:])
    with pytest.raises(ValueError, match="action"):
        env.check_errors()
    env.check_errors()  # cleared
    with pytest.raises(ValueError, match="tile id"):
        env.reset(init_grids=np.full((3, 4, 5), 9, np.uint8))
        env.check_errors()
    env.close()


def test_dirty_workspace_does_not_matter():
    z, kw = load("narrow_8x20_p300")
    env = make(kw, 2, [int(z["seed"])] * 2)
    env._workspace.fill_(0x0101010101010101)
    replay_fixture(env, NS_fixture(z, 60), (0, 1))
    env.close()


class NS_fixture(dict):
    """the first `steps` steps of a fixture"""

    def __init__(self, z, steps):
        super().__init__({k: z[k] for k in z.files})
        for k in ("actions", "pos", "stats", "reward", "done", "iteration", "changes", "obs_crc"):
            self[k] = self[k][:steps]
        keep = self["full_steps"] < steps
        for k in ("full_steps", "full_map", "full_obs"):
            self[k] = self[k][keep]


def test_captured_step_replays_across_an_episode_end():
    z, kw = load("narrow_4x5")
    n = 3
    env = make(kw, n, [int(z["seed"])] * n)
    actions = torch.zeros(n, dtype=torch.int32, device=DEV)
    env.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the usual warm-up before a capture; the env is re-seeded below
        env.step(actions)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = env.step(actions)
    env.seed([int(z["seed"])] * n)

    def step(a):
        actions.copy_(a)
        graph.replay()
        return out

    replay_fixture(env, z, (0, 2), step=step)  # 140 steps: two automatic resets inside replayed launches
    env.close()
