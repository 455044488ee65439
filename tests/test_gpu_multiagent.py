"""Multi-agent turtle stepping (include/pcgrl_amd_multiagent.h) on the GPU: every episode recorded from the reference
(tests/golden/multiagent/, tools/gen_golden_multiagent.py) through MultiAgentVecEnv from the seed and with injected maps and
positions, every (lanes per env, mask width) kernel form against the numpy statement of the rules (tests/multiagent_rules.py) at
every sub-step over several auto-reset episodes, the episode end, the occupancy channel on both row-store paths, out-of-range
actions, checkpoints, graph capture, a side stream, the refusals and the single-env adapter."""
import ctypes as C
import glob
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest

import multiagent_rules as mr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "multiagent", "*.npz")))
NAMES = [os.path.basename(f)[:-4] for f in FIXTURES]


def _env(problem, shape, n, A, show, seeds, **kw):
    from control_pcgrl_amd import MultiAgentVecEnv
    return MultiAgentVecEnv(problem, shape, n, A, show_agents=show, device="cuda:0", seeds=seeds, **kw)


def _rules(problem, shape, A, show, seeds, **kw):
    return [mr.MultiAgentRules(problem, shape, A, show_agents=show, seed=int(s), **kw) for s in seeds]


def _random_actions(rng, n, A, nt, p_absent):
    a = np.where(rng.random((n, A)) < 0.5, rng.integers(0, 4, (n, A)), 4 + rng.integers(0, nt, (n, A)))
    return np.where(rng.random((n, A)) < p_absent, -1, a).astype(np.int32)


class Driver:
    """an engine and one MultiAgentRules per env, stepped together and compared"""

    def __init__(self, env, rules):
        self.env, self.rules, self.n, self.A = env, rules, env.num_envs, env.n_agents
        self.resets = 0
        self.split_rounds = 0  # rounds that left some agents of an env done and others not

    def reset(self, **kw):
        obs, _ = self.env.reset(**kw)
        grids, pos = kw.get("init_grids"), kw.get("init_pos")
        want = np.stack([r.reset(None if grids is None else grids[i], None if pos is None else pos[i])
                         for i, r in enumerate(self.rules)])
        assert np.array_equal(obs.cpu().numpy(), want), "reset observations"
        self.check_state()

    def check_state(self):
        st = self.env.get_state()
        assert np.array_equal(st.grids.cpu().numpy(), np.stack([r.grid for r in self.rules])), "maps"
        assert np.array_equal(st.agent_pos.cpu().numpy(), np.array([r.pos for r in self.rules])), "positions"
        assert np.array_equal(st.agent_done.cpu().numpy(), np.array([r.done for r in self.rules])), "done bits"
        assert np.array_equal(st.iteration.cpu().numpy(), [r.iteration for r in self.rules])
        assert np.array_equal(st.changes.cpu().numpy(), [r.changes for r in self.rules])
        assert np.array_equal(st.stats.cpu().numpy(), np.stack([r.stats for r in self.rules]))

    def step(self, actions, check_obs=True, env_step=None):
        """one round of every env against the rules; returns the envs that were reset"""
        env = self.env
        before = env._obs.clone() if check_obs else None
        a = torch.from_numpy(np.ascontiguousarray(actions, dtype=np.int32)).to(env.device)
        obs, rew, done, trunc, info = (env_step or env.step)(a)
        rew, done, stats, done_all = (t.cpu().numpy() for t in (rew, done, info["stats"], info["done_all"]))
        obs = obs.cpu().numpy() if check_obs else None
        reset_envs = []
        for i, r in enumerate(self.rules):
            n_eps = len(r.episodes)
            o, w_rew, w_done, w_stats, w_all, _ = r.step(actions[i], auto_reset=env.auto_reset)
            assert np.array_equal(stats[i], w_stats), ("stats", i, stats[i], w_stats)
            assert np.array_equal(rew[i], w_rew.astype(np.float32)), ("reward", i, rew[i], w_rew)
            assert np.array_equal(done[i], w_done), ("done", i)
            assert bool(done_all[i]) == w_all, ("done_all", i)
            self.split_rounds += int(w_done.any() and not w_done.all())
            if len(r.episodes) > n_eps:
                reset_envs.append(i)
            if check_obs:
                for k in range(self.A):  # a row without a sub-step keeps what it held
                    want = o[k] if o[k] is not None else before[i, k].cpu().numpy()
                    assert np.array_equal(obs[i, k], want), ("observation", i, k)
        self.resets += len(reset_envs)
        return reset_envs

    def check_last_episode(self, envs):
        le = self.env.last_episode()
        ret, ln, fs, ne = (t.cpu().numpy() for t in (le.ep_return, le.ep_len, le.final_stats, le.n_episodes))
        for i in envs:
            w_ret, w_len, w_stats = self.rules[i].episodes[-1]
            assert ln[i] == w_len and np.array_equal(fs[i], w_stats) and ne[i] == len(self.rules[i].episodes), i
            assert abs(ret[i] - w_ret) <= 1e-9 * max(1.0, abs(w_ret)), (i, ret[i], w_ret)  # (float64 sums in the same order)


# ---- the recorded reference episodes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_fixture_from_the_seed_and_injected(path):
    """env 0 replays the file (its seed, its actions) and is held against the file itself; the other envs take random actions
    and are held against the numpy rules.  Then the first episode again from the file's first map and positions, injected."""
    z = np.load(path)
    kw = mr.fixture_kwargs(z)
    problem, shape, A, show = kw["problem"], kw["map_shape"], kw["n_agents"], kw["show_agents"]
    cp, nt, n = kw["change_percentage"], mr.po.N_TILES[kw["problem"]], 5
    seeds = np.array([int(z["meta_seed"])] + [900 + k for k in range(n - 1)])
    rounds = list(mr.fixture_rounds(z))
    rng = np.random.default_rng(5)
    full = {int(s): k for k, s in enumerate(z["full_idx"])}
    for injected in (False, True):
        env = _env(problem, shape, n, A, show, seeds, change_percentage=cp, auto_reset=not injected)
        d = Driver(env, _rules(problem, shape, A, show, seeds, change_percentage=cp))
        if injected:
            g = rng.integers(0, nt, (n,) + shape).astype(np.uint8)
            p = np.stack([rng.integers(0, shape[0], (n, A)), rng.integers(0, shape[1], (n, A))], axis=-1).astype(np.int32)
            g[0], p[0] = z["reset_map"][0], z["reset_pos"][0]
            d.reset(init_grids=g, init_pos=p)
        else:
            d.reset()
        assert np.array_equal(env._obs[0].cpu().numpy(), z["reset_obs"][0])
        ep = 0
        for r, (acts, subs, reset_after) in enumerate(rounds):
            a = _random_actions(rng, n, A, nt, 0.1)
            a[0] = acts
            done_before = list(d.rules[0].done)
            reset_envs = d.step(a, check_obs=(r % 3 == 0 or reset_after or r < 3))
            # env 0 against the file: the sub-steps of this round
            stats, rew, done = (t[0].cpu().numpy() for t in (env._stats, env._reward, env._done))
            for s in subs:
                i = int(z["sub_agent"][s])
                assert not done_before[i]
                assert np.array_equal(stats[i], z["stats"][s]) and rew[i] == np.float32(z["reward"][s]) and done[i] == z["done"][s], s
                if not (reset_after and not injected):
                    assert mr.crc(env._obs[0, i].cpu().numpy()) == int(z["obs_crc"][s]), ("observation", s)
                    if int(s) in full:
                        assert np.array_equal(env._obs[0, i].cpu().numpy(), z["full_obs"][full[int(s)]])
            if len(subs) and not (reset_after and not injected):
                st = env.get_state()
                assert mr.crc(st.grids[0].cpu().numpy()) == int(z["map_crc"][subs[-1]])
                assert np.array_equal(st.agent_pos[0].cpu().numpy(), z["pos"][subs[-1]])
                assert int(st.iteration[0]) == int(z["iteration"][subs[-1]]) and int(st.changes[0]) == int(z["changes"][subs[-1]])
            if reset_after:
                assert bool(env._done_all[0])
                if injected:
                    break
                assert 0 in reset_envs
                ep += 1
                if ep < len(z["reset_map"]):
                    assert np.array_equal(env._obs[0].cpu().numpy(), z["reset_obs"][ep])
                    assert np.array_equal(env.get_state().grids[0].cpu().numpy(), z["reset_map"][ep])
                    assert np.array_equal(env.agent_positions()[0].cpu().numpy(), z["reset_pos"][ep])
                d.check_last_episode(reset_envs)
        d.check_state()
        env.check_errors()
        env.close()


# ---- every kernel form -----------------------------------------------------------------------------------------------------------
# (lanes per env, mask bits): 8x8 (8, 32), 16x16 (16, 32; the compile-time encoder), 20x24 (32, 32), 40x16 (64, 32),
# 12x40 (32, 64), 40x48 (64, 64); odd batch sizes leave the last wavefront partly filled
FORMS = [("binary", (8, 8), 3, True, 0.1, 77), ("zelda", (8, 8), 2, False, 0.1, 77),
         ("binary", (16, 16), 2, False, 0.03, 70), ("zelda", (16, 16), 3, True, 0.03, 70),
         ("binary", (20, 24), 3, False, 0.01, 37), ("zelda", (20, 24), 2, True, 0.01, 37),
         ("binary", (40, 16), 2, True, 0.01, 35), ("zelda", (40, 16), 3, False, 0.01, 35),
         ("binary", (12, 40), 3, True, 0.01, 37), ("zelda", (12, 40), 2, False, 0.01, 37),
         ("binary", (40, 48), 2, False, 0.003, 35), ("zelda", (40, 48), 3, True, 0.003, 35)]


@pytest.mark.parametrize("problem,shape,A,show,cp,n", FORMS,
                         ids=[f"{p}_{s[0]}x{s[1]}_a{a}{'_show' if sh else ''}" for p, s, a, sh, _, _ in FORMS])
def test_every_form_against_the_rules_over_auto_reset_episodes(problem, shape, A, show, cp, n):
    seeds = 300 + np.arange(n)
    env = _env(problem, shape, n, A, show, seeds, change_percentage=cp)
    d = Driver(env, _rules(problem, shape, A, show, seeds, change_percentage=cp))
    d.reset()
    rng, nt = np.random.default_rng(8), mr.po.N_TILES[problem]
    r = 0
    while min(len(x.episodes) for x in d.rules) < 3:
        assert r < 400
        reset_envs = d.step(_random_actions(rng, n, A, nt, 0.15), check_obs=(r % 4 == 0))
        if reset_envs:  # every reset: the new episode's first observations, its state, the latched episode
            want = np.stack([np.stack([d.rules[i].observation(k) for k in range(A)]) for i in reset_envs])
            assert np.array_equal(env._obs[reset_envs].cpu().numpy(), want)
            d.check_last_episode(reset_envs)
        if r % 4 == 0 or reset_envs:
            d.check_state()
        r += 1
    assert d.split_rounds > 0
    # the totals of pcgrl_reduce_episodes: return = the sum over the agents, length = iteration
    red = env.reduce_episodes().cpu().numpy()
    eps = [e for x in d.rules for e in x.episodes]
    assert red[2] == len(eps) and red[1] == sum(e[1] for e in eps)
    assert abs(red[0] - sum(e[0] for e in eps)) <= 1e-9 * max(1.0, sum(abs(e[0]) for e in eps))
    assert np.array_equal(red[3:], np.sum([e[2] for e in eps], axis=0))
    assert np.array_equal(env.observe().cpu().numpy(), np.stack([np.stack([x.observation(k) for k in range(A)]) for x in d.rules]))
    env.check_errors()
    env.close()


# ---- the episode end ------------------------------------------------------------------------------------------------------------------
def test_agents_finish_in_different_rounds_and_the_reset_lands_in_the_last():
    """5 x 7, three agents: max_iterations = 106 is no multiple of 3, so round 36 ends with agents 1 and 2 done and agent 0
    not; round 37 -- agent 0 alone, the others ignored whatever their action -- ends the episode at iteration 109"""
    n, A, shape = 9, 3, (5, 7)
    seeds = 40 + np.arange(n)
    env = _env("binary", shape, n, A, True, seeds)
    d = Driver(env, _rules("binary", shape, A, True, seeds))
    d.reset()
    rng = np.random.default_rng(3)
    for r in range(35):
        assert d.step(_random_actions(rng, n, A, 2, 0.0), check_obs=(r % 5 == 0)) == []
    assert d.step(_random_actions(rng, n, A, 2, 0.0)) == []
    assert env._done.cpu().numpy().tolist() == [[0, 1, 1]] * n and not env._done_all.any()
    assert np.array_equal(env.agents_done().cpu().numpy(), [[False, True, True]] * n)
    a = _random_actions(rng, n, A, 2, 0.0)
    assert d.step(a) == list(range(n))
    assert env._done.cpu().numpy().tolist() == [[1, 1, 1]] * n and env._done_all.all()
    assert all(x.episodes[-1][1] == 109 for x in d.rules)
    d.check_last_episode(range(n))
    d.check_state()  # (the new episode: counters 0, nobody done)
    assert not env.agents_done().any()
    env.close()


def test_without_auto_reset_a_finished_env_stays_as_it_is():
    n, A, shape = 6, 2, (2, 2)
    seeds = 50 + np.arange(n)
    env = _env("binary", shape, n, A, False, seeds, auto_reset=False)
    d = Driver(env, _rules("binary", shape, A, False, seeds))
    d.reset()
    rng = np.random.default_rng(4)
    for r in range(9):
        d.step(_random_actions(rng, n, A, 2, 0.0))
    assert env._done_all.all() and d.resets == 0
    before = env.get_state().grids.clone()
    d.step(_random_actions(rng, n, A, 2, 0.0))  # nobody takes a sub-step any more
    assert torch.equal(env.get_state().grids, before) and not env._reward.any()
    mask = np.array([1, 0, 1, 0, 0, 1], np.uint8)  # a masked reset restarts only its envs
    obs, _ = env.reset(mask=mask)
    for i in np.nonzero(mask)[0]:
        assert np.array_equal(obs[i].cpu().numpy(), d.rules[i].reset())
    d.check_state()
    env.close()


# ---- the occupancy channel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,shape", [("binary", (8, 8)), ("zelda", (8, 8)), ("binary", (5, 7)), ("zelda", (5, 7)),
                                           ("zelda", (16, 16)), ("binary", (12, 40))])
def test_occupancy_rows_corners_and_shared_cells(problem, shape):
    """8 x 8 -> 16-wide windows, rows of 16 x C bytes (binary 64, zelda 160: the 16-byte-chunk path); 5 x 7 -> 14-wide windows,
    rows of 56 and 140 bytes (the byte-string path).  Six agents: one in every corner of the map, so that the crop hangs off
    every edge, and two on one cell."""
    n, A = 11, 6
    H, W = shape
    nt = mr.po.N_TILES[problem]
    seeds = 60 + np.arange(n)
    env = _env(problem, shape, n, A, True, seeds)
    assert env.obs_shape == (2 * H, 2 * W, nt + 2)
    d = Driver(env, _rules(problem, shape, A, True, seeds))
    rng = np.random.default_rng(6)
    g = rng.integers(0, nt, (n, H, W)).astype(np.uint8)
    p = np.zeros((n, A, 2), np.int32)
    p[:, :4] = [[0, 0], [0, W - 1], [H - 1, 0], [H - 1, W - 1]]
    p[:, 4] = p[:, 5] = [H // 2, W // 2]
    d.reset(init_grids=g, init_pos=p)
    obs = env._obs.cpu().numpy()
    assert (obs[..., -1].reshape(n, A, -1).sum(axis=2) == 5).all()  # five occupied cells, all inside every window
    assert (obs[:, 0, :H, :, 0] == 1).all() and (obs[:, 3, H + 1:, :, 0] == 1).all()  # out of bounds above / below
    for r in range(6):
        d.step(_random_actions(rng, n, A, nt, 0.2))
    d.check_state()
    env.check_errors()
    env.close()


# ---- actions outside the action space ----------------------------------------------------------------------------------------------------
def test_out_of_range_actions_edit_nothing_and_raise_the_error_bit():
    n, A, shape = 10, 3, (8, 8)
    seeds = 80 + np.arange(n)
    env = _env("binary", shape, n, A, False, seeds)
    d = Driver(env, _rules("binary", shape, A, False, seeds))
    d.reset()
    rng = np.random.default_rng(7)
    d.step(_random_actions(rng, n, A, 2, 0.1))
    env.check_errors()
    a = _random_actions(rng, n, A, 2, 0.1)
    a[3, 1], a[7, 0] = 6, -5  # Discrete(4 + 2) ends at 5; -1 alone means absent
    d.step(a)  # (the rules: the sub-step counts, nothing is edited, nobody moves)
    d.check_state()
    with pytest.raises(ValueError):
        env.check_errors()
    d.step(_random_actions(rng, n, A, 2, 0.1))
    env.check_errors()  # (the bit was cleared by the poll)
    env.close()


def test_injected_positions_outside_the_map_and_unknown_tiles_are_made_safe_and_reported():
    """reset(init_pos) and load_state_dict: a position outside the map is clamped to it (the encoders index rows by it); a tile
    id the problem does not have reads as tile 0; both raise the error bit.  numpy actions are taken as they are."""
    n, A, shape = 6, 2, (8, 8)
    seeds = 85 + np.arange(n)
    env = _env("binary", shape, n, A, True, seeds)
    d = Driver(env, _rules("binary", shape, A, True, seeds))
    rng = np.random.default_rng(12)
    g = rng.integers(0, 2, (n,) + shape).astype(np.uint8)
    p = rng.integers(0, 8, (n, A, 2)).astype(np.int32)
    bad_g, bad_p = g.copy(), p.copy()
    bad_g[2, 3, 4], g[2, 3, 4] = 7, 0
    bad_p[1, 0], p[1, 0] = (-3, 99), (0, 7)
    bad_p[4, 1], p[4, 1] = (8, -1), (7, 0)
    obs, _ = env.reset(init_grids=bad_g, init_pos=bad_p)
    want = np.stack([r.reset(g[i], p[i]) for i, r in enumerate(d.rules)])
    assert np.array_equal(obs.cpu().numpy(), want)
    d.check_state()
    with pytest.raises(ValueError):
        env.check_errors()
    out = env.step(_random_actions(rng, n, A, 2, 0.0) * 0)  # (a numpy array; everybody moves up)
    for r in d.rules:
        r.step([0] * A)
    d.check_state()
    env.check_errors()
    sd = env.state_dict()
    sd["multiagent"]["pos"] = sd["multiagent"]["pos"].clone()
    sd["multiagent"]["pos"][3, 1] = torch.tensor([100, -100], dtype=torch.int32)
    env.load_state_dict(sd)
    d.rules[3].pos[1] = [7, 0]
    assert np.array_equal(env.observe().cpu().numpy(), np.stack([np.stack([r.observation(k) for k in range(A)]) for r in d.rules]))
    d.check_state()
    with pytest.raises(ValueError):
        env.check_errors()
    assert out[0] is env._obs
    env.close()


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,show", [("binary", True), ("zelda", False)])
def test_state_dict_into_a_fresh_engine_mid_episode_with_one_agent_done(problem, show):
    n, A, shape = 13, 3, (5, 7)
    nt = mr.po.N_TILES[problem]
    seeds = 90 + np.arange(n)
    env = _env(problem, shape, n, A, show, seeds)
    env.reset()
    rng = np.random.default_rng(9)
    for r in range(36):  # 106 iterations allowed: after 36 rounds of three, agents 1 and 2 are done and agent 0 is not
        env.step(torch.from_numpy(_random_actions(rng, n, A, nt, 0.0)).cuda())
    assert np.array_equal(env.agents_done().cpu().numpy(), [[False, True, True]] * n)
    sd = env.state_dict()
    other = _env(problem, shape, n, A, show, seeds + 1000)
    other.reset()
    other.load_state_dict(sd)
    assert torch.equal(other.observe(), env.observe().clone())
    for r in range(12):  # through the end of the episode, the reset inside the launch and into the next episode
        a = torch.from_numpy(_random_actions(rng, n, A, nt, 0.1)).cuda()
        out_a, out_b = env.step(a), other.step(a)
        for x, y in zip(out_a[:3] + (out_a[4]["stats"], out_a[4]["done_all"]), out_b[:3] + (out_b[4]["stats"], out_b[4]["done_all"])):
            assert torch.equal(x, y), r
    assert torch.equal(env.get_state().grids, other.get_state().grids)
    assert torch.equal(env.agent_positions(), other.agent_positions())
    assert torch.equal(env.last_episode().n_episodes, other.last_episode().n_episodes) and int(env.last_episode().n_episodes.min()) == 1
    with pytest.raises(ValueError):
        _env(problem, shape, n, 2, False, seeds).load_state_dict(sd)
    for e in (env, other):
        e.check_errors()
        e.close()


# ---- capture and streams ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,shape,show", [("binary", (16, 16), False), ("zelda", (12, 40), True)])
def test_a_round_captured_in_a_graph_and_replayed(problem, shape, show):
    n, A = 33, 2
    nt = mr.po.N_TILES[problem]
    seeds = 110 + np.arange(n)
    env = _env(problem, shape, n, A, show, seeds, change_percentage=0.02)
    d = Driver(env, _rules(problem, shape, A, show, seeds, change_percentage=0.02))
    d.reset()
    rng = np.random.default_rng(10)
    for _ in range(3):  # (eager warm-up before the capture)
        d.step(_random_actions(rng, n, A, nt, 0.1))
    static_a = torch.zeros((n, A), dtype=torch.int32, device=env.device)
    snapshot = env.state_dict()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = env.step(static_a)
    torch.cuda.current_stream().wait_stream(side)
    env.load_state_dict(snapshot)  # (a capture runs nothing; the state is the snapshot's either way)

    def replay(a):
        static_a.copy_(a)
        graph.replay()
        return out

    for r in range(30):
        d.step(_random_actions(rng, n, A, nt, 0.1), env_step=replay)
    d.check_state()
    assert d.resets > 0  # (the reset inside the captured launch, too)
    env.check_errors()
    env.close()


def test_on_a_side_stream():
    n, A, shape = 21, 3, (8, 8)
    seeds = 120 + np.arange(n)
    env = _env("zelda", shape, n, A, True, seeds, change_percentage=0.1)
    d = Driver(env, _rules("zelda", shape, A, True, seeds, change_percentage=0.1))
    side = torch.cuda.Stream()
    rng = np.random.default_rng(11)
    with torch.cuda.stream(side):
        d.reset()
        for r in range(25):
            d.step(_random_actions(rng, n, A, 8, 0.1))
        d.check_state()
    side.synchronize()
    env.check_errors()
    env.close()


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def test_attach_refusals_and_the_single_agent_entry_points_of_an_attached_engine():
    from control_pcgrl_amd import MultiAgentVecEnv, VecPcgrlEnv, _lib
    L = _lib.lib()

    def attach(env, A, show=0):
        rc = L.pcgrl_ma_attach(env._h, A, show)
        return rc, L.pcgrl_last_error().decode()

    for kw, word in ((dict(problem="binary", representation="narrow"), "turtle"), (dict(problem="binary", representation="wide"), "turtle"),
                     (dict(problem="sokoban", representation="turtle"), "binary and zelda"),
                     (dict(problem="binary", representation="turtle", static_prob=0.1), "static tiles"),
                     (dict(problem="zelda", representation="turtle", controls=["regions"]), "control metrics")):
        env = VecPcgrlEnv(map_shape=(8, 8), num_envs=4, **kw)
        rc, msg = attach(env, 2)
        assert rc == 2 and word in msg, (kw, msg)
        assert L.pcgrl_ma_attached(env._h) == 0
        env.reset()  # (still a single-agent engine)
        env.close()
    env = VecPcgrlEnv("minecraft_3D_maze", "turtle", (5, 5, 5), 4)
    assert attach(env, 2)[0] == 2
    env.close()
    env = VecPcgrlEnv("binary", "narrow", (8, 8), 4, act_window=(2, 2))
    assert attach(env, 2)[0] == 2
    env.close()
    env = VecPcgrlEnv("binary", "turtle", (8, 8), 4)
    assert attach(env, 1, 1) == (2, attach(env, 1, 1)[1]) and "more than one agent" in attach(env, 1, 1)[1]
    assert attach(env, 0)[0] == 1 and attach(env, 9)[0] == 1
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    assert L.pcgrl_ma_step(env._h, p, 1, p, p, p, p, p, None) == 1 and "not attached" in L.pcgrl_last_error().decode()
    assert attach(env, 2)[0] == 0 and L.pcgrl_ma_attached(env._h) == 1
    assert attach(env, 2)[0] == 1  # once
    # injected maps and positions come together
    assert L.pcgrl_ma_reset(env._h, None, p, None, None, None) == 1 and L.pcgrl_ma_reset(env._h, None, None, p, None, None) == 1
    assert L.pcgrl_ma_reset(env._h, None, None, None, None, None) == 0
    for name, args in (("pcgrl_step", (p, 1, p, p, p, p, None)), ("pcgrl_step_ex", (p, 1, p, p, p, p, p, None, None)),
                       ("pcgrl_step_seq", (p, 4, 1, 0, 1, 1, p, p, p, p, None)), ("pcgrl_rollout", (p, 2, 1, p, 0, p, p, p, None)),
                       ("pcgrl_rollout_ex", (p, 2, 1, p, 0, p, None, p, p, None, None)), ("pcgrl_update", (p, p, None)),
                       ("pcgrl_reset", (None, None, None, None)), ("pcgrl_observe", (p, None))):
        assert getattr(L, name)(env._h, *args) == 1, name
        assert "pcgrl_ma_attach" in L.pcgrl_last_error().decode(), name
    # what keeps working
    st = env.get_state()
    assert st.grids.shape == (4, 8, 8) and env.get_rng_state().shape == (4, 10)
    assert env.paths().length.shape == (4,) and env.last_episode().n_episodes.sum() == 0
    env.check_errors()
    env.close()
    with pytest.raises(NotImplementedError, match="more than one agent"):
        MultiAgentVecEnv("binary", (8, 8), 4, 1, show_agents=True)
    with pytest.raises(NotImplementedError, match="binary and zelda"):
        MultiAgentVecEnv("sokoban", (8, 8), 4, 2)


# ---- the single-env adapter ------------------------------------------------------------------------------------------------------------
def test_make_env_gives_the_reference_dict_shapes_and_replays_a_fixture():
    from control_pcgrl_amd import make_env, make_vec_env, MultiAgentVecEnv
    z = np.load(os.path.join(GOLDEN, "multiagent", "binary_5x7_a3_absent.npz"))
    cfg = NS(representation="turtle", max_board_scans=3, change_percentage=None, n_aux_tiles=0, show_agents=False, controls=None,
             act_window=None, static_prob=None, n_static_walls=None,
             task=NS(problem="binary", map_shape=(5, 7), obs_window=(10, 14), weights=None), multiagent=NS(n_agents=3))
    vec = make_vec_env(cfg, 4)
    assert isinstance(vec, MultiAgentVecEnv) and vec.n_agents == 3 and not vec.show_agents
    vec.close()
    env = make_env(cfg)
    o, r, dn, _, _ = env.step({"agent_1": 0})  # before any reset(): the engine's initial state, not an AttributeError
    assert list(o) == list(r) == ["agent_1"] and dn["__all__"] is False
    env.seed(int(z["meta_seed"]))
    obs, info = env.reset()
    assert sorted(obs) == ["agent_0", "agent_1", "agent_2"] and info == {}
    assert all(o.dtype == np.float32 and o.shape == (10, 14, 3) for o in obs.values())
    assert np.array_equal(np.stack([obs[k] for k in sorted(obs)]), z["reset_obs"][0])
    done = [False] * 3
    for acts, subs, reset_after in mr.fixture_rounds(z):
        action = {f"agent_{i}": int(a) for i, a in enumerate(acts) if a >= 0 and not done[i]}  # as RLlib: none after done
        o, r, d, t, inf = env.step(action)
        assert sorted(o) == sorted(r) == sorted(inf) == sorted(action) and sorted(d) == sorted(t) == sorted(list(action) + ["__all__"])
        for s in subs:
            k = f"agent_{int(z['sub_agent'][s])}"
            assert r[k] == np.float32(z["reward"][s]) and d[k] == bool(z["done"][s]) and mr.crc(o[k].astype(np.uint8)) == z["obs_crc"][s]
            assert list(inf[k].values()) == z["stats"][s].tolist() and list(inf[k]) == ["regions", "path-length"]
            done[int(z["sub_agent"][s])] = d[k]
        assert d["__all__"] == all(d[k] for k in action)
        if reset_after:
            break
    assert all(done)
    with pytest.raises(IndexError):
        env.step({"agent_0": 6})
    env.close()
