"""Open-loop rollouts of Super Mario Bros environments (SmbVecEnv.rollout / sample_actions, include/pcgrl_amd_smb_rollout.h):
K steps in one launch are bit for bit K step() calls.  The reference's recorded episodes of tests/golden/smb_env go through one
launch; rollouts are cut into chunks and mixed with step(); twin envs on maps of their own compare every output row, the
exported state and the episode totals; and the API's corners: batch sizes, auto_reset=False, an action outside the space in the
middle of a sequence, actions drawn on the device, captured rollouts, refusals."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smb_levels as sl  # noqa: E402
import smb_rules as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smb_env")
FIXTURES = ["narrow_4x5", "turtle_5x7_cp02", "narrow_8x20_p300", "turtle_8x20_p300", "narrow_6x12_win5x9", "turtle_5x7_alt",
            "narrow_16x116", "turtle_16x116"]
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


def tiled(actions, n):
    """actions [T] for every one of n envs -> int32 [T, n] on the device"""
    return torch.as_tensor(np.repeat(np.asarray(actions, dtype=np.int32)[:, None], n, axis=1), device=DEV)


def check_rows(out, z, rows, t0=0):
    """every per-step field of fixture z from step t0 on against the rows of a rollout with want_obs="all", on the envs `rows`"""
    r, d, s = out.reward.cpu().numpy(), out.done.cpu().numpy(), out.stats.cpu().numpy()
    o = out.obs.cpu().numpy()
    assert r.dtype == np.float64 and out.truncated is out.done
    full = {int(t): k for k, t in enumerate(z["full_steps"])}
    for k in range(r.shape[0]):
        t = t0 + k
        for i in rows:
            assert r[k, i] == z["reward"][t], (t, i, r[k, i], z["reward"][t])  # float64, bit for bit
            assert bool(d[k, i]) == bool(z["done"][t]), (t, i)
            assert s[k, i].tolist() == z["stats"][t].tolist(), (t, i)
            assert crc(o[k, i]) == int(z["obs_crc"][t]), (t, i)
            if t in full:
                assert np.array_equal(o[k, i], z["full_obs"][full[t]]), (t, i)


def check_state(env, z, t, rows):
    """get_state() after step t of the fixture: the position, the counters and, at a full step, the map"""
    st = env.get_state()
    full = {int(x): k for k, x in enumerate(z["full_steps"])}
    for i in rows:
        assert st.pos[i].tolist() == z["pos"][t].tolist(), (t, i)
        want = (0, 0) if z["done"][t] else (int(z["iteration"][t]), int(z["changes"][t]))
        assert (int(st.iteration[i]), int(st.changes[i])) == want, (t, i)
        if t in full:
            assert np.array_equal(st.grids[i].cpu().numpy(), z["full_map"][full[t]]), (t, i)


# ------------------------------------------------------------------------------------- 1. reference episodes, one launch

@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_through_one_launch(name):
    z, kw = load(name)
    seeds, T = [int(z["seed"]), 999, int(z["seed"])], len(z["actions"])
    env = make(kw, 3, seeds)
    obs, _ = env.reset()
    assert crc(obs[0].cpu().numpy()) == int(z["obs0_crc"]) == crc(obs[2].cpu().numpy())
    out = env.rollout(tiled(z["actions"], 3), want_obs="all")
    assert out.reward.shape == (T, 3) and out.stats.shape == (T, 3, 9) and out.obs.shape == (T, 3) + env.obs_shape
    assert torch.equal(out.actions, tiled(z["actions"], 3))
    check_rows(out, z, (0, 2))
    check_state(env, z, T - 1, (0, 2))  # T - 1 is a full step of every fixture: the final map too
    assert T - 1 in z["full_steps"]
    ends = int(z["done"].sum())
    assert out.episodes.count.tolist()[0] == ends and out.episodes.count.tolist()[2] == ends
    le = env.last_episode()
    assert le.count.tolist()[0] == ends
    if ends:
        last = int(np.nonzero(z["done"])[0][-1])
        assert le.stats[0].tolist() == z["stats"][last].tolist() and int(le.length[0]) == int(z["iteration"][last])
        ended = z["done"].astype(bool)
        assert int(out.episodes.length_sum[0]) == int(z["iteration"][ended].sum())
        assert out.episodes.stats_sum[0].tolist() == z["stats"][ended].astype(np.int64).sum(0).tolist()
    env.check_errors()
    # the maps at the full steps in between: a second env, one launch up to each of them
    cuts = [int(t) for t in z["full_steps"] if 0 <= t < T - 1]
    if cuts:
        env2 = make(kw, 3, seeds)
        env2.reset()
        start = 0
        for t in cuts:
            o = env2.rollout(tiled(z["actions"][start:t + 1], 3), want_obs="last")
            check_state(env2, z, t, (0, 2))
            assert crc(o.obs[0].cpu().numpy()) == int(z["obs_crc"][t])
            start = t + 1
        env2.close()
    env.close()


# ------------------------------------------------------------------------------------------------- 2. chunked and mixed

@pytest.mark.parametrize("name", ["narrow_4x5", "turtle_5x7_cp02"])
def test_chunks_and_steps_in_between_equal_one_launch(name):
    """rollouts of 1, 7 and 64 steps and the rest, each but the last followed by one step()"""
    z, kw = load(name)
    seeds, T, acts = [int(z["seed"])] * 2, len(z["actions"]), z["actions"]
    whole = make(kw, 2, seeds)
    whole.reset()
    ref = whole.rollout(tiled(acts, 2), want_obs="none")
    assert ref.obs is None
    env = make(kw, 2, seeds)
    env.reset()
    t, ends = 0, 0
    for size in (1, 7, 64, None):
        size = T - t if size is None else size
        out = env.rollout(tiled(acts[t:t + size], 2), want_obs="last")
        assert torch.equal(out.reward, ref.reward[t:t + size]) and torch.equal(out.done, ref.done[t:t + size])
        assert torch.equal(out.stats, ref.stats[t:t + size])
        assert out.reward[:, 0].tolist() == z["reward"][t:t + size].tolist()
        ends += int(out.episodes.count[0])
        t += size
        o = out.obs.cpu().numpy()
        assert out.obs.shape == (2,) + env.obs_shape and crc(o[0]) == int(z["obs_crc"][t - 1]) == crc(o[1])
        check_state(env, z, t - 1, (0, 1))
        if t == T:
            break
        obs, rew, done, _, info = env.step(torch.full((2,), int(acts[t]), dtype=torch.int32, device=DEV))
        assert rew.tolist() == [float(z["reward"][t])] * 2 and done.tolist() == [bool(z["done"][t])] * 2
        assert info["stats"][0].tolist() == z["stats"][t].tolist() and crc(obs[1].cpu().numpy()) == int(z["obs_crc"][t])
        ends += int(done[0])
        t += 1
    assert t == T and ends == int(z["done"].sum()) == int(ref.episodes.count[0])
    assert torch.equal(env.export_state(), whole.export_state())  # maps, records, counters, both streams
    env.check_errors()
    env.close()
    whole.close()


# ----------------------------------------------------------------------------------------- 3. twin envs on own maps

def own_maps(n=65, h=8, w=30, steps=30, power=300):
    rng = np.random.default_rng(5)
    grids = sl.batch(3, n, h, w)  # structured, random and walled levels
    pos = np.stack([rng.integers(0, h, n), rng.integers(0, w, n)], axis=1)
    # mostly writes, so that solidity-changing, solidity-keeping and no-change edits all occur in every env
    actions = np.where(rng.random((steps, n)) < 0.25, rng.integers(0, 4, (steps, n)), rng.integers(4, 11, (steps, n)))
    kw = dict(representation="turtle", map_shape=(h, w), solver_power=power)
    return kw, grids, pos, torch.as_tensor(actions.astype(np.int32), device=DEV)


def step_rows(env, actions):
    """K step() calls -> the rows a rollout returns, and the episode totals accumulated from last_episode() after each done"""
    K, n = actions.shape
    rows = dict(reward=[], done=[], stats=[], obs=[])
    count = np.zeros(n, np.int32)
    ret = np.zeros(n, np.float64)
    length = np.zeros(n, np.int64)
    stats = np.zeros((n, 9), np.int64)
    for k in range(K):
        obs, rew, done, _, info = env.step(actions[k])
        for key, v in (("reward", rew), ("done", done), ("stats", info["stats"]), ("obs", obs)):
            rows[key].append(v.clone())
        d = done.cpu().numpy()
        if d.any():
            le = env.last_episode()
            count += d
            ret = np.where(d, ret + le.ep_return.cpu().numpy(), ret)  # in the order the episodes finished
            length += np.where(d, le.length.cpu().numpy(), 0)
            stats += np.where(d[:, None], le.stats.cpu().numpy(), 0)
    return {k: torch.stack(v) for k, v in rows.items()}, (count, ret, length, stats)


def assert_same_rows(out, rows):
    assert torch.equal(out.reward, rows["reward"]) and torch.equal(out.done, rows["done"])  # float64 rewards: bit for bit
    assert torch.equal(out.stats, rows["stats"]) and torch.equal(out.obs, rows["obs"])


def assert_same_episodes(ep, totals):
    count, ret, length, stats = totals
    assert ep.count.cpu().numpy().tolist() == count.tolist()
    assert ep.return_sum.cpu().numpy().tobytes() == ret.tobytes()  # bit for bit
    assert ep.length_sum.cpu().numpy().tolist() == length.tolist() and ep.stats_sum.cpu().numpy().tolist() == stats.tolist()


def test_twin_envs_on_own_maps():
    kw, grids, pos, actions = own_maps()
    n = grids.shape[0]
    # a small change budget, so that episodes end (and the next ones are drawn) inside the launch
    A = make(kw, n, np.arange(n), change_percentage=0.03)
    B = make(kw, n, np.arange(n), change_percentage=0.03)
    A.reset(init_grids=grids, init_pos=pos)
    B.reset(init_grids=grids, init_pos=pos)
    rows, totals = step_rows(A, actions)
    out = B.rollout(actions, want_obs="all")
    assert_same_rows(out, rows)
    assert torch.equal(out.actions, actions)
    assert torch.equal(A.export_state(), B.export_state())
    assert_same_episodes(out.episodes, totals)
    ends = totals[0]
    assert ends.sum() > n // 2 and ends.max() >= 2  # several ends inside the launch, and more than one in some env
    st = B.get_state()
    assert n < int(st.searches.sum()) < n * (actions.shape[0] + 1)  # some edits searched, and not all of them
    B.check_errors()
    A.close()
    B.close()


# --------------------------------------------------------------------------------------------------- 4. batch sizes

@pytest.fixture(scope="module")
def narrow_4x5():
    return load("narrow_4x5")


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_batch_sizes_and_batch_positions(n, narrow_4x5):
    z, kw = narrow_4x5
    env = make(kw, n, [int(z["seed"])] * n)
    env.reset()
    out = env.rollout(tiled(z["actions"][:80], n), want_obs="all")  # across the first automatic reset
    for t in (out.reward, out.done, out.stats, out.obs):
        assert (t == t[:, :1]).all()
    check_rows(out, z, (0, n - 1))
    assert z["done"][:80].sum() == 1 and out.episodes.count.tolist() == [1] * n
    env.check_errors()
    env.close()


# ------------------------------------------------------------------------------------------------ 5. auto_reset=False

def test_without_auto_reset_the_episode_goes_on(narrow_4x5):
    z, kw = narrow_4x5
    seeds = [int(z["seed"])] * 2
    actions = tiled(z["actions"][:66], 2)
    A = make(kw, 2, seeds, auto_reset=False)
    B = make(kw, 2, seeds, auto_reset=False)
    A.reset()
    B.reset()
    rows, totals = step_rows(A, actions)
    out = B.rollout(actions, want_obs="all")
    assert_same_rows(out, rows)
    assert torch.equal(A.export_state(), B.export_state())
    assert out.episodes.count.tolist() == [5, 5]  # done at every step from iteration 62 on, latched each time
    assert_same_episodes(out.episodes, totals)
    assert B.get_state().iteration.tolist() == [66, 66] and out.done[:, 0].tolist() == [False] * 61 + [True] * 5
    A.close()
    B.close()


# ------------------------------------------------------------------------------------------------------ 6. a bad action

def test_a_bad_action_in_the_middle_of_a_sequence():
    kw = dict(representation="narrow", map_shape=(4, 5))
    seeds = [1, 2, 3]
    good = np.random.default_rng(2).integers(0, 7, (8, 3)).astype(np.int32)
    bad = good.copy()
    bad[3, 1], bad[5, 2] = 7, -1
    env = make(kw, 3, seeds)
    env.reset()
    out = env.rollout(bad, want_obs="all")
    # a solo env per row steps the valid actions only; at a bad step its row is what the rule says: the env as it is
    rows = {i: [] for i in range(3)}
    for i in range(3):
        solo = make(kw, 1, [seeds[i]])
        solo.reset()
        for k in range(8):
            if not 0 <= bad[k, i] < 7:
                st = solo.get_state()
                rows[i].append((0.0, False, st.stats[0].tolist(), solo.observe()[0].clone()))
                continue
            obs, rew, done, _, info = solo.step(torch.tensor([int(bad[k, i])], dtype=torch.int32, device=DEV))
            rows[i].append((float(rew[0]), bool(done[0]), info["stats"][0].tolist(), obs[0].clone()))
        final = solo.get_state()
        st = env.get_state()
        assert torch.equal(st.grids[i], final.grids[0]) and st.pos[i].tolist() == final.pos[0].tolist()
        assert int(st.iteration[i]) == int(final.iteration[0]) == 8 - int((bad[:, i] != good[:, i]).sum())
        assert float(st.ep_return[i]) == float(final.ep_return[0]) and int(st.searches[i]) == int(final.searches[0])
        solo.close()
    for i in range(3):
        for k in range(8):
            rew, done, stats, obs = rows[i][k]
            assert float(out.reward[k, i]) == rew and bool(out.done[k, i]) == done, (k, i)
            assert out.stats[k, i].tolist() == stats and torch.equal(out.obs[k, i], obs), (k, i)
    # the bad rows themselves: reward 0, not done, and the env unchanged across them
    for k, i in ((3, 1), (5, 2)):
        assert float(out.reward[k, i]) == 0.0 and not bool(out.done[k, i])
        assert torch.equal(out.stats[k, i], out.stats[k - 1, i]) and torch.equal(out.obs[k, i], out.obs[k - 1, i])
        assert not torch.equal(out.obs[k + 1, i], out.obs[k, i])  # later steps proceed (narrow: the position moves on)
    assert torch.equal(out.actions, torch.as_tensor(bad, device=DEV))
    with pytest.raises(ValueError, match="action"):
        env.check_errors()
    env.check_errors()  # raised once
    env.close()


# ----------------------------------------------------------------------------------------------------- 7. drawn actions

def test_drawn_actions_equal_sample_then_step():
    from control_pcgrl_amd.smb_env import sampled_actions
    kw, grids, pos, _ = own_maps(n=65)
    n, s, K = 65, 77, 20
    A = make(kw, n, np.arange(n), change_percentage=0.03)
    B = make(kw, n, np.arange(n), change_percentage=0.03)
    A.reset(init_grids=grids, init_pos=pos)
    B.reset(init_grids=grids, init_pos=pos)
    assert A.num_actions == 11
    for first in (0, K):  # the second call continues at draw K
        taken = []
        rows = dict(reward=[], done=[], stats=[], obs=[])
        for k in range(K):
            a = A.sample_actions(seed=s)
            taken.append(a.clone())
            obs, rew, done, _, info = A.step(a)
            for key, v in (("reward", rew), ("done", done), ("stats", info["stats"]), ("obs", obs)):
                rows[key].append(v.clone())
        out = B.rollout(n_steps=K, seed=s, want_obs="all")
        assert torch.equal(out.actions, torch.stack(taken))
        assert np.array_equal(out.actions.cpu().numpy(), sampled_actions(s, first, K, n, 11))
        assert_same_rows(out, {k: torch.stack(v) for k, v in rows.items()})
        assert torch.equal(A.export_state(), B.export_state())
    own = torch.empty(n, dtype=torch.int32, device=DEV)
    assert B.sample_actions(seed=5, out=own) is own
    assert np.array_equal(own.cpu().numpy(), sampled_actions(5, 2 * K, 1, n, 11)[0])
    with pytest.raises(ValueError, match="out"):
        B.sample_actions(out=torch.empty(n + 1, dtype=torch.int32, device=DEV))
    B.check_errors()
    A.close()
    B.close()


# ----------------------------------------------------------------------------------------------------------- 8. capture

def capture(call, warm_up=None):
    """the usual warm-up on a side stream, then the capture of `call`; the caller puts the env's state right afterwards"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (warm_up or call)()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    return graph, out


def test_captured_rollout_replays_across_an_episode_end(narrow_4x5):
    z, kw = narrow_4x5
    n, K = 3, 35
    env = make(kw, n, [int(z["seed"])] * n)
    env.reset()
    actions = torch.zeros((K, n), dtype=torch.int32, device=DEV)
    graph, out = capture(lambda: env.rollout(actions, want_obs="all"))
    env.seed([int(z["seed"])] * n)
    env.reset()
    ends = 0
    for t0 in range(0, 140, K):  # four replays; the fixture's episodes end at steps 62 and 124
        actions.copy_(tiled(z["actions"][t0:t0 + K], n))
        graph.replay()
        check_rows(out, z, (0, 2), t0=t0)
        assert out.episodes.count.tolist() == [int(z["done"][t0:t0 + K].sum())] * n
        ends += int(out.episodes.count[0])
    assert ends == 2
    check_state(env, z, 139, (0, 2))
    env.check_errors()
    env.close()


def test_captured_drawn_rollout_draws_anew_at_every_replay():
    from control_pcgrl_amd.smb_env import sampled_actions
    kw, grids, pos, _ = own_maps(n=65)
    n, s, K = 65, 11, 6
    A = make(kw, n, np.arange(n), change_percentage=0.03)
    B = make(kw, n, np.arange(n), change_percentage=0.03)
    # the warm-up is a rollout of the same form with GIVEN actions: it makes the buffers and leaves the draw counter at 0.
    # The twin takes it too: the search counters of the state image count from the env's creation
    given = torch.zeros((K, n), dtype=torch.int32, device=DEV)
    for env in (A, B):
        env.reset(init_grids=grids, init_pos=pos)
    A.rollout(given, want_obs="last")
    graph, out = capture(lambda: B.rollout(n_steps=K, seed=s, want_obs="last"),
                         warm_up=lambda: B.rollout(given, want_obs="last"))
    for env in (A, B):
        env.seed(np.arange(n))
        env.reset(init_grids=grids, init_pos=pos)
    for rep in range(2):  # draws 0 .. K - 1, then K .. 2K - 1
        graph.replay()
        assert np.array_equal(out.actions.cpu().numpy(), sampled_actions(s, rep * K, K, n, 11)), rep
        ref = A.rollout(n_steps=K, seed=s, want_obs="last")  # the uncaptured twin
        for key in ("actions", "reward", "done", "stats", "obs"):
            assert torch.equal(getattr(out, key), getattr(ref, key)), (rep, key)
        assert torch.equal(out.episodes.count, ref.episodes.count)
        assert torch.equal(A.export_state(), B.export_state())
    B.check_errors()
    A.close()
    B.close()


# --------------------------------------------------------------------------------------------------------- 9. refusals

def test_refusals():
    from control_pcgrl_amd import SmbReadyVecEnv
    kw = dict(representation="narrow", map_shape=(4, 5))
    env = make(kw, 2, [1, 2])
    env.reset()
    with pytest.raises(ValueError, match="at least one step"):
        env.rollout(n_steps=0)
    with pytest.raises(ValueError, match="at least one step"):
        env.rollout(torch.zeros((0, 2), dtype=torch.int32, device=DEV))
    L = env._L
    r = torch.zeros(64, dtype=torch.float64, device=DEV)
    args = lambda n_steps=1, obs=None, mode=0: (env._handle(), None, 0, n_steps, 1, obs, mode, None, r.data_ptr()) + (None,) * 8  # noqa: E731
    assert L.pcgrl_smb_env_rollout(*args(n_steps=0)) == 1 and b"n_steps" in L.pcgrl_last_error()
    assert L.pcgrl_smb_env_rollout(*args(mode=3)) == 1 and b"obs_mode" in L.pcgrl_last_error()
    assert L.pcgrl_smb_env_rollout(*args(mode=1)) == 1 and b"16-byte" in L.pcgrl_last_error()
    assert L.pcgrl_smb_env_rollout(*args(obs=env._obs.data_ptr() + 8, mode=2)) == 1 and b"16-byte" in L.pcgrl_last_error()
    assert L.pcgrl_smb_env_rollout(*args(n_steps=2 ** 30 + 1)) == 1 and b"2^31" in L.pcgrl_last_error()
    assert L.pcgrl_smb_env_num_actions(env._handle()) == 7
    assert int(env.get_state().iteration.sum()) == 0  # nothing was launched
    assert L.pcgrl_smb_env_rollout(*args()) == 0  # every other output null
    assert env.get_state().iteration.tolist() == [1, 1]
    env.close()
    ready = SmbReadyVecEnv(num_envs=2, device=DEV, seeds=[1, 2], solver_budget=4, **kw)
    ready.reset()
    with pytest.raises(NotImplementedError, match="solver budget"):
        ready.rollout(n_steps=3)
    assert L.pcgrl_smb_env_rollout(ready._handle(), None, 0, 3, 1, None, 0, *([None] * 10)) == 1
    assert b"solver budget" in L.pcgrl_last_error()
    while int(ready.env_busy().sum()):
        ready.step_ready(torch.zeros(2, dtype=torch.int32, device=DEV))
    ready.set_solver_budget(0)
    before = ready.get_state().iteration.clone()
    out = ready.rollout(n_steps=3, want_obs="none")  # the base class's from here on
    assert out.obs is None and (ready.get_state().iteration - before).tolist() == [3, 3]
    assert L.pcgrl_smb_env_num_actions(ready._handle()) == 7
    ready.close()
