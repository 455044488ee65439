"""Asynchronous stepping of Super Mario Bros environments on the device (SmbReadyVecEnv, include/pcgrl_amd_smb_ready.h) against
the launch rules of tests/smb_ready_rules.py and the fixtures of tests/golden/smb_env.

The harness keeps a progress counter per env and feeds env i the action it is due -- only when the device said it is not busy.
After every launch it compares the status bytes, the observation rows and the committed state with the rules; at every EMITTED
it compares reward (float64, exact), done and statistics, and on fixture rows every recorded field of the fixture."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smb_env_rules as E  # noqa: E402
import smb_levels as sl  # noqa: E402
import smb_ready_rules as RR  # noqa: E402
import smb_rules as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smb_env")
DEV = "cuda:0"
EMITTED, BUSY = RR.EMITTED, RR.BUSY
_EVALUATIONS = {}


class RememberingRules(E.SmbEnvRules):
    """the rules' play-through of a level is computed once for all the tests and budgets that meet the level"""

    def _evaluate(self):
        key = (self.grid.shape, self.grid.tobytes(), self.power)
        if key not in _EVALUATIONS:
            _EVALUATIONS[key] = R.get_stats(self.grid, self.power)
        self.searches += 1
        stats, rec = _EVALUATIONS[key]
        self.stats, self.rec = list(stats), rec


class Rules(RR.SmbReadyRules):
    env_class = RememberingRules


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes()) & 0xFFFFFFFF


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cp = float(z["change_percentage"])
    kw = dict(representation=str(z["representation"]), map_shape=tuple(int(s) for s in z["map_shape"]),
              obs_window=tuple(int(s) for s in z["obs_window"]), weights={k: float(w) for k, w in zip(R.STAT_KEYS, z["weights"])},
              change_percentage=None if cp < 0 else cp, solver_power=int(z["solver_power"]))
    return z, kw


def rules_kw(kw):
    out = {k: v for k, v in kw.items() if k != "map_shape"}
    out["shape"] = kw["map_shape"]
    return out


def make(kw, n, seeds, budget, **more):
    from control_pcgrl_amd import SmbReadyVecEnv
    return SmbReadyVecEnv(num_envs=n, device=DEV, seeds=seeds, reward_dtype=torch.float64, solver_budget=budget, **kw, **more)


class Harness:
    """env: an SmbReadyVecEnv; rules: one Rules per env; feed(i, k): the k-th action env i consumes; fixtures: {row: z}"""

    def __init__(self, env, rules, feed, fixtures=None, fixture_steps=None, auto_reset=True, step=None, check_state=True):
        self.env, self.rules, self.feed, self.fixtures = env, rules, feed, fixtures or {}
        self.fixture_steps = fixture_steps  # how many of a fixture's steps the feed follows (all without a number)
        self.auto_reset, self.check_state = auto_reset, check_state
        self.step = step or env.step_ready
        self.n = env.num_envs
        self.progress = [0] * self.n   # actions consumed
        self.emitted = [0] * self.n    # transitions emitted
        self.busy = None               # what the device said after the last launch
        self.launches = 0
        self.largest_budget = 0
        self.seen_status = set()
        self.base = None               # the env's counters before the harness's first reset: they count since the create

    def _compare_state(self):
        st = self.env.get_state()
        grids, pos = st.grids.cpu().numpy(), st.pos.cpu().numpy()
        it, ch, stats = st.iteration.tolist(), st.changes.tolist(), st.stats.cpu().numpy()
        last_loss, searches = st.last_loss.cpu().numpy(), st.searches.tolist()
        total, most = st.search_iterations.tolist(), st.max_search_iterations.tolist()
        for i, r in enumerate(self.rules):
            c = r.committed()
            want_stats, want_loss = r.committed_stats()
            where = (self.launches, i)
            assert np.array_equal(grids[i], c.grid) and pos[i].tolist() == list(c.pos), where
            assert (it[i], ch[i]) == (c.iteration, c.changes), where
            assert stats[i].tolist() == want_stats and last_loss[i] == want_loss, where
            b_searches, b_total, b_most = self.base[i]
            assert searches[i] - b_searches == r.committed_searches and total[i] - b_total == r.iterations, where
            assert most[i] == max(b_most, r.max_per_launch) and r.max_per_launch <= self.largest_budget, where

    def reset(self, budget, mask=None, init_grids=None, init_pos=None):
        self.largest_budget = max(self.largest_budget, budget)
        if self.base is None:
            st = self.env.get_state()
            self.base = list(zip(st.searches.tolist(), st.search_iterations.tolist(), st.max_search_iterations.tolist()))
        obs, _ = self.env.reset(mask=mask, init_grids=init_grids, init_pos=init_pos)
        o = obs.cpu().numpy()
        for i, r in enumerate(self.rules):
            if mask is None or mask[i]:
                r.reset(budget, None if init_grids is None else init_grids[i], None if init_pos is None else init_pos[i])
                self.progress[i] = self.emitted[i]  # a dropped step's action is fed again: nothing of it happened
                assert np.array_equal(o[i], r.observation()), i
            else:  # untouched, parked search included; its row is the committed observation
                assert np.array_equal(o[i], r.committed().observation()), i
        self.busy = self.env.env_busy().cpu().numpy().astype(bool)
        assert self.busy.tolist() == [r.busy() for r in self.rules]
        if self.check_state:
            self._compare_state()

    def launch(self, budget, junk=0):
        """one step_ready launch at `budget` (the env's budget must be that); busy rows get the action `junk`"""
        self.largest_budget = max(self.largest_budget, budget)
        taking = [not b for b in self.busy]
        actions = [self.feed(i, self.progress[i]) if taking[i] else junk for i in range(self.n)]
        obs, rew, done, trunc, info = self.step(torch.tensor(actions, dtype=torch.int32, device=DEV))
        self.launches += 1
        status = info["status"].cpu().numpy()
        o = obs.cpu().numpy()
        rew, done, stats = rew.cpu().numpy(), done.cpu().numpy(), info["stats"].cpu().numpy()
        assert rew.dtype == np.float64
        for i, r in enumerate(self.rules):
            where = (self.launches, i, self.progress[i])
            want, out = r.launch(actions[i], budget, self.auto_reset)
            assert int(status[i]) == want, where + (int(status[i]), want)
            self.seen_status.add(want)
            assert np.array_equal(o[i], r.observation()), where
            self.progress[i] += int(taking[i])
            if out is None:
                continue
            k = self.emitted[i]
            assert k == self.progress[i] - 1, where  # the transition of the last action the env consumed
            self.emitted[i] += 1
            assert rew[i] == out["reward"] and bool(done[i]) == out["done"] and stats[i].tolist() == out["stats"], where
            z = self.fixtures.get(i)
            if z is not None and k < (self.fixture_steps or len(z["actions"])):
                assert rew[i] == z["reward"][k] and bool(done[i]) == bool(z["done"][k]), where
                assert stats[i].tolist() == z["stats"][k].tolist() and crc(o[i]) == int(z["obs_crc"][k]), where
                assert out["pos"] == z["pos"][k].tolist(), where
                assert (out["iteration"], out["changes"]) == (int(z["iteration"][k]), int(z["changes"][k])), where
                full = np.nonzero(z["full_steps"] == k)[0]
                if len(full):
                    assert np.array_equal(o[i], z["full_obs"][full[0]]), where
                    assert np.array_equal(r.env.grid, z["full_map"][full[0]]), where  # (the state check ties it to the device)
        self.busy = (status & BUSY) != 0
        assert self.busy.tolist() == [r.busy() for r in self.rules]
        if self.check_state or (status & EMITTED).any():
            self._compare_state()
        return status

    def run_until(self, budget, emitted, limit):
        """launches until every env has emitted `emitted` transitions"""
        while min(self.emitted) < emitted:
            self.launch(budget)
            assert self.launches <= limit, "the schedule does not advance"

    def drain(self, budget, limit=100000):
        while self.busy.any():
            before = self.launches
            # only envs with pending statistics are left alone by a drain: feed nothing new
            assert all(r.mode != RR.IDLE or not b for r, b in zip(self.rules, self.busy))
            self.launch(budget, junk=0)
            assert self.launches - before == 1 and self.launches <= limit


def fixture_harness(name, budget, n_steps=None, check_state=True, **more):
    z, kw = load(name)
    seed = int(z["seed"])
    env = make(kw, 3, [seed, 999, seed], budget, **more)
    rules = [Rules(seed=s, **rules_kw(kw)) for s in (seed, 999, seed)]
    acts = z["actions"] if n_steps is None else z["actions"][:n_steps]
    h = Harness(env, rules, lambda i, k: int(acts[k % len(acts)]), fixtures={0: z, 2: z}, fixture_steps=len(acts),
                check_state=check_state)
    return z, env, h, len(acts)


# ---------------------------------------------------------------------------------------- 1. fixtures from the seed alone

@pytest.mark.parametrize("name,budget", [("narrow_4x5", 1), ("narrow_4x5", 5), ("narrow_4x5", 16), ("narrow_4x5", 64),
                                         ("turtle_5x7_cp02", 7), ("turtle_5x7_cp02", 32), ("turtle_5x7_cp02", 200),
                                         ("narrow_8x20_p300", 64), ("narrow_8x20_p300", 1000), ("paint_8x30_p300", 100)])
def test_fixture_from_the_seed_alone(name, budget):
    """rows 0 and 2 against the fixture, row 1 (another seed) against the rules: the rows desynchronise"""
    z, env, h, steps = fixture_harness(name, budget, check_state=budget > 1)  # (at budget 1 the state at every EMITTED)
    h.reset(budget)
    full = np.nonzero(z["full_steps"] == -1)[0][0]
    st = env.get_state()
    for i in (0, 2):
        assert np.array_equal(st.grids[i].cpu().numpy(), z["full_map"][full]) and st.pos[i].tolist() == list(z["pos0"])
    h.run_until(budget, steps, limit=40 * steps + 4000)
    assert h.emitted[0] == h.emitted[2] >= steps
    longest = max(r.max_per_launch for r in h.rules)
    assert longest <= budget
    if budget <= 16:
        assert h.seen_status >= {EMITTED, BUSY}  # searches were parked
    ends = int(z["done"][:steps].sum())
    if h.emitted[0] == steps:
        assert env.last_episode().count.tolist()[0] == ends
    env.check_errors()
    env.close()


def test_pending_statistics_after_an_automatic_reset():
    """turtle_5x7_cp02 has ten episode ends: at budget 7 the new level's search outlasts the launch that drew it"""
    z, env, h, steps = fixture_harness("turtle_5x7_cp02", 7)
    h.reset(7)
    h.run_until(7, steps, limit=20000)
    assert (EMITTED | BUSY) in h.seen_status and 0 in h.seen_status and EMITTED in h.seen_status and BUSY in h.seen_status
    env.close()


# ------------------------------------------------------------- 2. a budget above every search is synchronous stepping, bit for bit

def test_a_large_budget_equals_synchronous_stepping():
    from control_pcgrl_amd import SmbVecEnv
    z, kw = load("narrow_6x12_win5x9")
    seeds = [int(z["seed"]), 31, 32]
    sync = SmbVecEnv(num_envs=3, device=DEV, seeds=seeds, reward_dtype=torch.float64, **kw)
    ready = make(kw, 3, seeds, 4 * kw["solver_power"])  # two passes of two searches fit in a launch
    o1, _ = sync.reset()
    o2, _ = ready.reset()
    assert torch.equal(o1, o2) and ready.env_busy().tolist() == [0, 0, 0]
    for t, a in enumerate(z["actions"][:80]):
        actions = torch.full((3,), int(a), dtype=torch.int32, device=DEV)
        o1, r1, d1, _, i1 = sync.step(actions)
        o2, r2, d2, _, i2 = ready.step_ready(actions)
        assert i2["status"].tolist() == [EMITTED] * 3, t
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(i1["stats"], i2["stats"]), t
        assert r2[0].item() == z["reward"][t]
        s1, s2 = sync.get_state(), ready.get_state()
        for f in ("grids", "pos", "iteration", "changes", "n_step", "searches", "stats", "last_loss", "ep_return",
                  "search_iterations"):
            assert torch.equal(getattr(s1, f), getattr(s2, f)), (t, f)
        # the most one launch spent: a launch that ends an episode runs two searches, which the synchronous count keeps apart
        assert (s2.max_search_iterations >= s1.max_search_iterations).all()
    e1, e2 = sync.last_episode(), ready.last_episode()
    assert torch.equal(e1.count, e2.count) and torch.equal(e1.ep_return, e2.ep_return) and torch.equal(e1.stats, e2.stats)
    sync.close()
    ready.close()


# ------------------------------------------------------------------------------------------- 3. own maps against the rules

def own_turtle(n, budget, emitted, h=8, w=30, power=300, seed=5):
    rng = np.random.default_rng(seed)
    grids = sl.batch(3, n, h, w)  # structured, random and walled levels
    pos = np.stack([rng.integers(0, h, n), rng.integers(0, w, n)], axis=1)
    kw = dict(representation="turtle", map_shape=(h, w), solver_power=power)
    env = make(kw, n, np.arange(n), budget)
    rules = [Rules(seed=i, **rules_kw(kw)) for i in range(n)]
    # mostly writes, so that solidity-changing, solidity-keeping and no-change edits all occur in every env
    acts = np.where(rng.random((emitted + 1, n)) < 0.25, rng.integers(0, 4, (emitted + 1, n)), rng.integers(4, 11, (emitted + 1, n)))
    hn = Harness(env, rules, lambda i, k: int(acts[k % len(acts), i]))
    hn.reset(budget, init_grids=grids, init_pos=pos)
    hn.run_until(budget, emitted, limit=60 * emitted)
    return env, hn


def test_own_maps_65_envs_turtle():
    env, h = own_turtle(65, 48, 30)
    assert h.seen_status >= {EMITTED, BUSY} and h.launches > 30
    st = env.get_state()
    assert int(st.max_search_iterations.max()) <= 48 and 65 < int(st.searches.sum())
    env.check_errors()
    env.close()


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_batch_sizes_and_batch_positions(n):
    """the same seed at every batch position gives the fixture's trajectory and the same schedule at every one of them"""
    z, kw = load("narrow_4x5")
    env = make(kw, n, [int(z["seed"])] * n, 5)
    rule = Rules(seed=int(z["seed"]), **rules_kw(kw))
    obs, _ = env.reset()
    rule.reset(5)
    busy = env.env_busy()
    assert (obs == obs[0]).all() and busy.tolist() == [int(rule.busy())] * n
    t = 0
    while t < 80:  # across the first automatic reset
        a = int(z["actions"][t])
        obs, rew, done, _, info = env.step_ready(torch.full((n,), a, dtype=torch.int32, device=DEV))
        want, out = rule.launch(a, 5)
        assert info["status"].tolist() == [want] * n and (obs == obs[0]).all(), t
        assert np.array_equal(obs[n - 1].cpu().numpy(), rule.observation())
        if out is not None:
            assert (rew == float(z["reward"][t])).all() and (done == bool(z["done"][t])).all(), t
            assert (info["stats"] == info["stats"][0]).all() and info["stats"][n - 1].tolist() == z["stats"][t].tolist()
            assert crc(obs[n - 1].cpu().numpy()) == int(z["obs_crc"][t])
            t += 1
    assert rule.launches > 80 and z["done"][:80].sum() == 1
    env.check_errors()
    env.close()


def test_own_maps_stock_size_narrow():
    h, w, n, budget = 16, 116, 4, 512
    rng = np.random.default_rng(6)
    grids = np.stack([sl.make("structured", 2, h, w), sl.make("structured", 1, h, w), sl.make("structured", 3, h, w),
                      sl.make("structured", 5, h, w)])
    kw = dict(representation="narrow", map_shape=(h, w))
    env = make(kw, n, np.arange(n), budget)
    rules = [Rules(seed=i, **rules_kw(kw)) for i in range(n)]
    acts = rng.integers(0, 7, (13, n))
    hn = Harness(env, rules, lambda i, k: int(acts[k % 13, i]))
    hn.reset(budget, init_grids=grids)
    hn.run_until(budget, 12, limit=2000)
    st = env.get_state()
    assert int(st.max_search_iterations.max()) <= budget < int(st.search_iterations.max()) and BUSY in hn.seen_status
    env.check_errors()
    env.close()


# ------------------------------------------------------------------------------------------------------------ 4. resets

def busy_mix(budget=3, n=8):
    """n turtle envs of 5 x 7 with frequent episode ends, stepped until pending steps and pending statistics are both in flight"""
    kw = dict(representation="turtle", map_shape=(5, 7), change_percentage=0.2)
    env = make(kw, n, 40 + np.arange(n), budget)
    rules = [Rules(seed=40 + i, **rules_kw(kw)) for i in range(n)]
    acts = np.random.default_rng(2).integers(4, 11, (64, n))  # writes only: many searches
    h = Harness(env, rules, lambda i, k: int(acts[k % 64, i]))
    h.reset(budget)
    for _ in range(400):
        modes = [r.mode for r in rules]
        if modes.count(RR.PENDING_STEP) >= 2 and modes.count(RR.PENDING_STATS) >= 1:
            return env, h, modes
        h.launch(budget)
    raise AssertionError("no launch left both kinds of parked search")


def test_masked_reset_abandons_what_was_in_flight():
    env, h, modes = busy_mix()
    steps = [i for i, m in enumerate(modes) if m == RR.PENDING_STEP]
    stats = [i for i, m in enumerate(modes) if m == RR.PENDING_STATS]
    mask = [0] * h.n
    mask[steps[0]] = mask[stats[0]] = 1  # one of each; the other pending step (steps[1]) goes on
    before = env.get_state()
    h.reset(3, mask=mask)  # compares the selected rows with a fresh episode, the others with their committed state
    st = env.get_state()
    assert (int(st.iteration[steps[0]]), int(st.changes[steps[0]])) == (0, 0)
    assert torch.equal(st.grids[steps[1]], before.grids[steps[1]]) and h.rules[steps[1]].mode == RR.PENDING_STEP
    h.run_until(3, max(h.emitted) + 6, limit=3000)  # everyone continues: the abandoned step left no trace
    env.check_errors()
    env.close()


def test_reset_with_injected_maps_while_searches_are_parked():
    env, h, modes = busy_mix()
    grids = sl.batch(3, h.n, 5, 7)
    pos = np.stack([np.arange(h.n) % 5, np.arange(h.n) % 7], axis=1)
    mask = [int(m != RR.IDLE) for m in modes]
    mask[modes.index(RR.PENDING_STEP)] = 0  # one pending step is left alone
    h.reset(3, mask=mask, init_grids=grids, init_pos=pos)
    h.run_until(3, max(h.emitted) + 6, limit=3000)
    h.reset(3, init_grids=grids, init_pos=pos)  # and all of them
    h.run_until(3, max(h.emitted) + 3, limit=3000)
    env.check_errors()
    env.close()


def test_without_auto_reset_the_episode_goes_on():
    z, kw = load("narrow_4x5")
    seed = int(z["seed"])
    env = make(kw, 2, [seed] * 2, 5, auto_reset=False)
    rules = [Rules(seed=seed, **rules_kw(kw)) for _ in range(2)]
    h = Harness(env, rules, lambda i, k: int(z["actions"][k]), auto_reset=False)
    h.reset(5)
    h.run_until(5, 66, limit=3000)
    st = env.get_state()
    assert st.iteration.tolist() == [66, 66] and (EMITTED | BUSY) not in h.seen_status
    assert env.last_episode().count.tolist() == [5, 5]  # done at every step from iteration 62 on, latched each time
    env.close()


# --------------------------------------------------------------------------------------- 5. the budget changes between launches

def test_budget_changed_with_searches_parked():
    z, env, h, steps = fixture_harness("turtle_5x7_cp02", 4)
    h.reset(4)
    changed_while_busy = 0
    schedule = [4] * 9 + [50] * 3 + [3] * 11
    while min(h.emitted) < steps:
        b = schedule[h.launches % len(schedule)]
        if b != env.solver_budget:
            changed_while_busy += int(h.busy.any())
            env.set_solver_budget(b)
        h.launch(b)
        assert h.launches < 20000
    assert changed_while_busy >= 3 and h.largest_budget == 50
    assert int(env.get_state().max_search_iterations.max()) <= 50
    env.close()


# ------------------------------------------------------------------------------------------ 6. actions outside the space

def test_action_outside_the_space():
    z, env, h, steps = fixture_harness("narrow_8x20_p300", 8)
    h.reset(8)
    while not h.busy.any():
        h.launch(8)
    while h.busy.any():  # busy rows get an action outside the space: it is not looked at
        h.launch(8, junk=99)
    env.check_errors()  # no error bit
    assert min(h.emitted) > 0
    # the same action on idle rows: the error bit, and the envs as they were
    before = env.get_state()
    obs0 = env._obs.clone()
    obs, rew, done, _, info = env.step_ready(torch.full((3,), 99, dtype=torch.int32, device=DEV))
    assert info["status"].tolist() == [EMITTED] * 3 and rew.tolist() == [0.0] * 3 and done.tolist() == [False] * 3
    st = env.get_state()
    assert torch.equal(obs, obs0) and torch.equal(st.grids, before.grids) and torch.equal(st.iteration, before.iteration)
    assert torch.equal(info["stats"], before.stats)
    with pytest.raises(ValueError, match="action"):
        env.check_errors()
    env.check_errors()  # cleared
    env.close()


# ------------------------------------------------------------------------------------------------------ 7. dirty memory

def test_dirty_workspace_does_not_matter():
    z, env, h, steps = fixture_harness("narrow_8x20_p300", 64, n_steps=60)
    env._workspace.fill_(0x0101010101010101)
    h.reset(64)
    h.run_until(64, steps, limit=5000)
    assert BUSY in h.seen_status
    assert int(env.get_state().max_search_iterations.max()) <= 64 == h.largest_budget
    env.close()


# ---------------------------------------------------------------------------------------------------------- 8. capture

def test_captured_launch_replays_across_an_episode_end():
    z, kw = load("narrow_4x5")
    seed, n = int(z["seed"]), 3
    env = make(kw, n, [seed, 999, seed], 6)
    actions = torch.zeros(n, dtype=torch.int32, device=DEV)
    env.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the usual warm-up before a capture; the env is re-seeded and reset below
        env.step_ready(actions)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = env.step_ready(actions)
    env.seed([seed, 999, seed])

    def step(a):  # the actions tensor is updated in place; the harness fills it from the status of the previous replay
        actions.copy_(a)
        graph.replay()
        return out

    rules = [Rules(seed=s, **rules_kw(kw)) for s in (seed, 999, seed)]
    h = Harness(env, rules, lambda i, k: int(z["actions"][k % 140]), fixtures={0: z, 2: z}, fixture_steps=140, step=step)
    h.reset(6)  # abandons whatever the warm-up and the capture left parked
    h.run_until(6, 80, limit=5000)  # across the first automatic reset, with searches parked at both ends of it
    assert z["done"][:80].sum() == 1 and h.seen_status >= {EMITTED, BUSY, EMITTED | BUSY}
    env.check_errors()
    env.close()


# ------------------------------------------------------------------------------------------------------ 9. mode changes

def test_mode_changes():
    z, env, h, steps = fixture_harness("narrow_8x20_p300", 8)
    assert env.solver_budget == 8 and env.park_bytes == 48 + 2112
    h.reset(8)
    with pytest.raises(RuntimeError, match="budget"):
        env.step(torch.zeros(3, dtype=torch.int32, device=DEV))
    from control_pcgrl_amd import _lib
    assert _lib.lib().pcgrl_smb_env_step(env._handle(), env._status.data_ptr(), 1, None, None, None, None, None, None) == 1
    while not h.busy.any():
        h.launch(8)
    with pytest.raises(ValueError, match="busy"):
        env.set_solver_budget(0)
    assert env.solver_budget == 8
    h.drain(8)
    env.set_solver_budget(0)
    assert env.solver_budget == 0 and env.env_busy().tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="budget"):
        env.step_ready(torch.zeros(3, dtype=torch.int32, device=DEV))
    # synchronous stepping from here on: the fixture rows go on where they were
    k = h.emitted[0]
    assert k == h.emitted[2] == h.progress[0]
    obs, rew, done, _, info = env.step(torch.full((3,), int(z["actions"][k]), dtype=torch.int32, device=DEV))
    assert rew[0].item() == z["reward"][k] and info["stats"][2].tolist() == z["stats"][k].tolist()
    assert crc(obs[0].cpu().numpy()) == int(z["obs_crc"][k])
    env.set_solver_budget(16)  # and back
    assert env.solver_budget == 16
    obs, rew, done, _, info = env.step_ready(torch.full((3,), int(z["actions"][k + 1]), dtype=torch.int32, device=DEV))
    assert set(info["status"].tolist()) <= {EMITTED, BUSY}
    env.close()
