"""Asynchronous stepping of minecraft_3D_maze (narrow): pcgrl_set_solver_budget / pcgrl_step_ready / pcgrl_env_busy on the
resumable path searches (csrc/async3d/pcgrl_async3d.h, include/pcgrl_amd_async3d.h), through the C ABI and against the oracle,
which steps an env exactly when the engine says it emitted a transition, with the action the env consumed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pcgrl_oracle as po  # noqa: E402  (checker only)

REW_TOL = 1e-6  # the suite's: float32 reward outputs against the oracle's float64
P3 = "minecraft_3D_maze"
EMITTED, BUSY = 1, 2


def _vec(*a, **k):
    from control_pcgrl_amd import VecPcgrlEnv
    return VecPcgrlEnv(*a, **k)


def _pair(shape, n, auto_reset, seeds=None, rep="narrow", **kw):
    seeds = np.arange(n) if seeds is None else seeds
    return (_vec(P3, rep, shape, n, seeds=seeds, auto_reset=auto_reset, **kw), po.OracleVecEnv(P3, rep, shape, n, seeds=seeds, **kw))


class Drive:
    """The loop of tests/test_gpu_round6.py::_drive_ready, kept between calls: consumed actions, busy flags, per-env counts."""

    def __init__(self, env, orc, n, auto_reset):
        self.env, self.orc, self.n, self.auto_reset = env, orc, n, auto_reset
        self.pend = np.zeros(n, np.int32)
        self.has_pend = np.zeros(n, bool)
        self.emitted_n = np.zeros(n, int)
        self.done_n = np.zeros(n, int)
        self.busy_launches = self.launches = self.seen_eb = self.seen_zero_after_eb = 0
        self.streak = np.zeros(n, int)
        self.max_streak = np.zeros(n, int)
        self.sync_busy()

    def sync_busy(self):
        self.busy = self.env.env_busy().cpu().numpy().astype(bool)
        self.has_pend[:] = False
        self.was_eb = np.zeros(self.n, bool)

    def launch(self, a, check_obs=True):
        n = self.n
        consume = ~self.busy
        self.pend[consume] = a[consume]
        self.has_pend[consume] = True
        obs, rew, done, _, info = self.env.step_ready(torch.as_tensor(a, dtype=torch.int32).cuda())
        status = info["status"].cpu().numpy()
        emitted = (status & EMITTED) != 0
        assert not (emitted & ~self.has_pend).any(), "a transition without a consumed action"
        oobs, orew, odone, ostats = self.orc.step_masked(emitted, self.pend, auto_reset=self.auto_reset)
        t = self.launches
        if emitted.any():
            assert np.array_equal(info["stats"].cpu().numpy()[emitted], ostats[emitted]), t
            assert np.abs(rew.cpu().numpy()[emitted] - orew[emitted]).max() <= REW_TOL, t
            assert np.array_equal(done.cpu().numpy()[emitted], odone[emitted]), t
            if check_obs:
                assert np.array_equal(obs.cpu().numpy()[emitted], oobs[emitted]), t
        self.has_pend[emitted] = False
        self.busy = (status & BUSY) != 0
        assert not (~self.busy & self.has_pend).any(), "an idle env still owes a transition"
        self.seen_eb += int((status == (EMITTED | BUSY)).sum())
        self.seen_zero_after_eb += int(((status == 0) & self.was_eb).sum())
        self.was_eb = (status == (EMITTED | BUSY)) | (self.was_eb & (status == BUSY))
        self.emitted_n += emitted
        self.done_n += emitted & odone
        self.busy_launches += int(self.busy.any())
        self.launches += 1
        self.streak = np.where(self.busy, self.streak + 1, 0)
        self.max_streak = np.maximum(self.max_streak, self.streak)
        return status, emitted, (obs, rew, done, info), (oobs, orew, odone, ostats)

    def final_state_equal(self):
        n = self.n
        idle = ~self.env.env_busy().cpu().numpy().astype(bool)
        st, ost = self.env.get_state(), self.orc.get_state()
        # (an env with a parked STEP shows the map before that step, which is the oracle's: it has not played it either)
        assert np.array_equal(st.grids.cpu().numpy().reshape(n, -1), ost["grids"])
        assert np.array_equal(st.stats.cpu().numpy()[idle], ost["stats"][idle])


def _run_until(d, rng, n_act, cap, min_emitted=20, need_done=False, check_obs_every=1):
    """launches until every env has emitted min_emitted transitions (an episode end among them if need_done); reaching the
    launch cap fails"""
    while True:
        if (d.emitted_n >= min_emitted).all() and (not need_done or (d.done_n >= 1).all()):
            break
        assert d.launches < cap, f"launch cap {cap} reached: min emitted {d.emitted_n.min()}, envs with an episode end {(d.done_n >= 1).sum()}"
        d.launch(rng.integers(0, n_act, size=d.n).astype(np.int32), check_obs=d.launches % check_obs_every == 0)
    print(f"launches {d.launches} (cap {cap}), emitted min {d.emitted_n.min()} total {d.emitted_n.sum()}, busy launches {d.busy_launches}, "
          f"longest busy streak {d.max_streak.max()}, EMITTED|BUSY seen {d.seen_eb}")


# ------------------------------------------------------------------------------------------------ 1
def test_budget_is_accepted_on_the_3d_maze():
    """fails before this feature: pcgrl_set_solver_budget on a 3-D maze engine returned PCGRL_EUNSUPPORTED"""
    n = 32
    env = _vec(P3, "narrow", (7, 7, 7), n, seeds=np.arange(n))
    env.set_solver_budget(8)
    env.reset()
    out = env.step_ready(torch.zeros(n, dtype=torch.int32).cuda())
    status = out[4]["status"].cpu().numpy()
    assert status.shape == (n,) and status.dtype == np.uint8 and (status <= 3).all()
    from control_pcgrl_amd import _lib
    assert int(env._L.pcgrl_park_bytes_per_env(env._h)) == 12320
    assert set(_lib.ASYNC3D_SYMBOLS) == {"pcgrl_park_bytes_per_env"}
    env.check_errors()


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("shape,n,launches", [((7, 7, 7), 256, 320), ((10, 10, 10), 48, 300)])
def test_large_budget_equals_synchronous_stepping(shape, n, launches):
    """a budget no step exceeds: every status byte is EMITTED alone and every output is bit-equal to pcgrl_step's"""
    kw = dict(change_percentage=0.05)  # episodes of a few dozen steps: the launches cross several episode ends
    a = _vec(P3, "narrow", shape, n, seeds=np.arange(n), auto_reset=True, **kw)
    b = _vec(P3, "narrow", shape, n, seeds=np.arange(n), auto_reset=True, **kw)
    a.set_solver_budget(1 << 20)
    a.reset()
    b.reset()
    assert int(a.env_busy().sum()) == 0
    g = torch.Generator().manual_seed(5)
    ends = 0
    for t in range(launches):
        act = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32).cuda()
        oa, ra, da, _, ia = a.step_ready(act)
        ob, rb, db, _, ib = b.step(act)
        assert int((ia["status"] != EMITTED).sum()) == 0, t
        assert torch.equal(ia["stats"], ib["stats"]) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(oa, ob), t
        ends += int(da.sum())
    assert ends >= n, "the launches were to cross episode ends"
    a.set_solver_budget(0)  # nobody is busy: back to synchronous stepping
    act = torch.zeros(n, dtype=torch.int32).cuda()
    oa, ra, da, _, ia = a.step(act)
    ob, rb, db, _, ib = b.step(act)
    assert torch.equal(ia["stats"], ib["stats"]) and torch.equal(ra, rb) and torch.equal(oa, ob)
    a.check_errors(); b.check_errors()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("shape,n,budget,auto_reset,cp,cap", [
    ((7, 7, 7), 256, 1, True, 0.05, 30000), ((7, 7, 7), 256, 4, True, 0.05, 12000), ((7, 7, 7), 256, 32, True, 0.05, 4000),
    ((7, 7, 7), 256, 1, False, 0.05, 30000), ((7, 7, 7), 256, 4, False, 0.05, 12000), ((7, 7, 7), 256, 32, False, 0.05, 4000),
    ((15, 15, 15), 6, 4, True, 0.004, 30000), ((6, 7, 8), 64, 4, True, 0.05, 12000)])
def test_parking_vs_oracle(shape, n, budget, auto_reset, cp, cap):
    """random actions under small budgets: searches park, busy envs ignore their actions, every emitted transition is the
    oracle's.  Runs until every env has emitted 20 transitions (and ended an episode where auto-reset is on); the launch cap
    only ends a run that would never get there, and reaching it fails."""
    env, orc = _pair(shape, n, auto_reset, change_percentage=cp)
    env.set_solver_budget(budget)
    env.reset()
    orc.reset()
    d = Drive(env, orc, n, auto_reset)
    _run_until(d, np.random.default_rng(11), 2, cap, need_done=auto_reset)
    assert d.busy_launches > 0, "no launch had a busy env: nothing parked"
    d.final_state_equal()
    env.check_errors()


# ------------------------------------------------------------------------------------------------ 4
def _serpentine():
    """7^3, DIRT except a flat corridor of 31 cells: AIR at heights 1 (feet) and 2 (head-room) over rows 0, 2, 4, 6 and one
    connecting cell between consecutive rows (index 0 of the array is the height)"""
    g = np.ones((7, 7, 7), np.uint8)
    for z in (1, 2):
        for y in (0, 2, 4, 6):
            g[z, y, :] = 0
        g[z, 1, 6] = g[z, 3, 0] = g[z, 5, 6] = 0
    return g


def test_search_parked_over_several_launches_by_construction():
    """budget 1 on a corridor whose pair of searches needs at least 4 trips (both searches pop all 31 cells, a trip pops at
    most 16 entries): the injected reset and a step that edits the corridor are busy for at least 2 launches each"""
    n = 16
    g = _serpentine()
    maps = np.broadcast_to(g, (n, 7, 7, 7)).copy()
    pos = np.broadcast_to(np.array([1, 6, 0], np.int32), (n, 3)).copy()
    # on the CPU: what the oracle says about the map and about the edit
    assert po.stats_for_grids(P3, maps[:1], (7, 7, 7)).tolist() == [[1, 31, 0]]
    probe = po.OracleVecEnv(P3, "narrow", (7, 7, 7), 1, seeds=[0])
    probe.reset(init_grids=maps[:1], init_pos=pos[:1])
    assert probe.step(np.array([1], np.int32))[3].tolist() == [[1, 30, 0]], "the edit at (1, 6, 0) moves the path length"

    env, orc = _pair((7, 7, 7), n, False)
    env.set_solver_budget(1)
    env.reset(init_grids=torch.as_tensor(maps), init_pos=torch.as_tensor(pos))
    orc.reset(init_grids=maps, init_pos=pos)
    d = Drive(env, orc, n, False)
    assert d.busy.all(), "the injected reset leaves every env waiting for its statistics"
    act = np.ones(n, np.int32)  # DIRT at the corridor's end
    # (a) the reset's statistics: busy for at least 2 launches, then 0 once (no transition: the oracle is not stepped)
    reset_launches = 0
    while d.busy.any():
        assert reset_launches < 2000
        status, emitted, _, _ = d.launch(act)
        assert not emitted.any()
        reset_launches += 1
    assert reset_launches >= 2 and (status == 0).all(), reset_launches
    assert np.array_equal(env.get_state().stats.cpu().numpy(), np.broadcast_to([1, 31, 0], (n, 3)))
    # (b) the step that edits the corridor: consumed now, busy for at least 2 launches, then emitted = the oracle's
    step_launches = 0
    while True:
        assert step_launches < 2000
        status, emitted, (obs, rew, done, info), (oobs, orew, odone, ostats) = d.launch(act)
        step_launches += 1
        if emitted.any():
            break
        assert (status == BUSY).all()
        # nothing of the unfinished step is committed
        assert np.array_equal(env.get_state().grids.cpu().numpy(), maps)
    assert emitted.all() and step_launches >= 3, step_launches  # (>= 2 busy launches before the emitting one)
    assert ostats.tolist() == [[1, 30, 0]] * n and np.array_equal(info["stats"].cpu().numpy(), ostats)
    print(f"reset: {reset_launches} launches, the edit: {step_launches} launches")
    # (c) re-inject the maps while steps are parked: the abandoned steps are never played
    for rep in range(3):
        env.reset(init_grids=torch.as_tensor(maps), init_pos=torch.as_tensor(pos))
        orc.reset(init_grids=maps, init_pos=pos)
        d.sync_busy()
        for k in range(reset_launches + 1 + rep):  # ... the reset's statistics, then into the parked step, one launch deeper each time
            d.launch(act)
        assert d.busy.all() and d.has_pend.all(), "the step is parked when the maps are injected again"
    env.reset(init_grids=torch.as_tensor(maps), init_pos=torch.as_tensor(pos))
    orc.reset(init_grids=maps, init_pos=pos)
    d.sync_busy()
    before = d.emitted_n.copy()
    for k in range(reset_launches + step_launches + 2):
        d.launch(act)
    assert ((d.emitted_n - before) >= 1).all()
    d.final_state_equal()
    env.check_errors()


# ------------------------------------------------------------------------------------------------ 5
def test_auto_reset_emitted_busy_then_zero():
    """a small budget after an episode end: EMITTED | BUSY (the transition and the new episode's first observation), then 0
    once when the new map's statistics are there"""
    n = 128
    env, orc = _pair((7, 7, 7), n, True, change_percentage=0.02)
    env.set_solver_budget(2)
    env.reset()
    orc.reset()
    d = Drive(env, orc, n, True)
    rng = np.random.default_rng(4)
    eb_obs_checked = 0
    while d.seen_eb < n or d.seen_zero_after_eb < n:
        assert d.launches < 20000, (d.seen_eb, d.seen_zero_after_eb)
        status, emitted, (obs, _, done, _), (oobs, _, odone, _) = d.launch(rng.integers(0, 2, size=n).astype(np.int32))
        eb = status == (EMITTED | BUSY)
        if eb.any():
            assert odone[eb].all(), "EMITTED | BUSY only at an episode end"
            assert np.array_equal(obs.cpu().numpy()[eb], oobs[eb])  # (the oracle's post-reset observation)
            eb_obs_checked += int(eb.sum())
    assert eb_obs_checked >= n
    d.final_state_equal()
    le, ole = env.last_episode(), orc.last_episode()
    assert np.array_equal(le.n_episodes.cpu().numpy(), ole["n_episodes"])
    assert np.array_equal(le.final_stats.cpu().numpy(), ole["final_stats"])
    env.check_errors()


# ------------------------------------------------------------------------------------------------ 6
def test_captured_chain_replays_to_the_eager_launches():
    """which launch an env advances in depends on the map, the action and the budget alone: T captured launches replay to
    the statuses, stats and rewards of T eager launches on a twin"""
    n, T, budget = 192, 120, 3
    kw = dict(change_percentage=0.03)
    a = _vec(P3, "narrow", (7, 7, 7), n, seeds=np.arange(n), auto_reset=True, **kw)
    b = _vec(P3, "narrow", (7, 7, 7), n, seeds=np.arange(n), auto_reset=True, **kw)
    for e in (a, b):
        e.set_solver_budget(budget)
        e.reset()
    g = torch.Generator().manual_seed(8)
    acts = torch.randint(0, 2, (T, n), generator=g, dtype=torch.int32).cuda()

    def bufs():
        return (torch.zeros((T, n), dtype=torch.float32, device="cuda"), torch.zeros((T, n), dtype=torch.uint8, device="cuda"),
                torch.zeros((T, n, 3), dtype=torch.int32, device="cuda"), torch.zeros((T, n), dtype=torch.uint8, device="cuda"))

    rew_a, done_a, stats_a, status_a = bufs()
    rew_b, done_b, stats_b, status_b = bufs()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            cap = torch.cuda.current_stream().cuda_stream
            for t in range(T):
                rc = a._L.pcgrl_step_ready(a._h, acts[t].data_ptr(), 1, None, rew_a[t].data_ptr(), done_a[t].data_ptr(),
                                           stats_a[t].data_ptr(), status_a[t].data_ptr(), cap)
                assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    s = torch.cuda.current_stream().cuda_stream
    for t in range(T):
        rc = b._L.pcgrl_step_ready(b._h, acts[t].data_ptr(), 1, None, rew_b[t].data_ptr(), done_b[t].data_ptr(), stats_b[t].data_ptr(),
                                   status_b[t].data_ptr(), s)
        assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(status_a, status_b)
    em = (status_b & EMITTED) != 0
    assert int(em.sum()) > 0 and int(((status_b & BUSY) != 0).sum()) > 0 and int((~em).sum()) > 0
    assert torch.equal(stats_a[em], stats_b[em]) and torch.equal(rew_a[em], rew_b[em]) and torch.equal(done_a[em], done_b[em])
    sa, sb = a.get_state(), b.get_state()
    assert torch.equal(sa.grids, sb.grids) and torch.equal(sa.counters, sb.counters)
    a.check_errors(); b.check_errors()


# ------------------------------------------------------------------------------------------------ 7
def test_checkpoint_with_parked_steps():
    """export with parked steps -> a fresh engine with the same budget continues exactly (parked searches are not in the
    image: they start again); an engine without a budget refuses the image before anything is overwritten"""
    n, budget = 96, 2
    kw = dict(change_percentage=0.05)
    env, orc = _pair((7, 7, 7), n, True, **kw)
    env.set_solver_budget(budget)
    env.reset()
    orc.reset()
    d = Drive(env, orc, n, True)
    rng = np.random.default_rng(21)
    while True:
        assert d.launches < 5000
        d.launch(rng.integers(0, 2, size=n).astype(np.int32))
        if d.launches >= 60 and (d.busy & d.has_pend).sum() >= 4:  # parked steps (not only resets waiting for statistics)
            break
    sd = env.state_dict()
    fresh = _vec(P3, "narrow", (7, 7, 7), n, seeds=1000 + np.arange(n), auto_reset=True, **kw)
    fresh.reset()
    before = fresh.get_state().grids.clone()
    with pytest.raises(ValueError):
        fresh.load_state_dict(sd)  # no budget: busy envs could not be finished
    assert torch.equal(fresh.get_state().grids, before), "refused before anything is overwritten"
    fresh.set_solver_budget(budget)
    fresh.load_state_dict(sd)
    assert np.array_equal(fresh.env_busy().cpu().numpy().astype(bool), d.busy)
    d2 = Drive(fresh, orc, n, True)
    d2.pend, d2.has_pend = d.pend.copy(), d.has_pend.copy()  # the actions the parked steps consumed travel with the image
    for t in range(200):
        d2.launch(rng.integers(0, 2, size=n).astype(np.int32))
    assert d2.emitted_n.sum() > n
    d2.final_state_equal()
    fresh.check_errors(); env.check_errors()


# ------------------------------------------------------------------------------------------------ 8
def test_refusals_leave_no_error_bit():
    n = 16
    env = _vec(P3, "narrow", (7, 7, 7), n, seeds=np.arange(n))
    env.set_solver_budget(4)
    env.reset()
    act = torch.zeros(n, dtype=torch.int32).cuda()
    with pytest.raises(ValueError):
        env.step(act)
    with pytest.raises(ValueError):
        env.rollout(torch.zeros((4, n), dtype=torch.int32).cuda())
    with pytest.raises(ValueError):
        env.update(act)
    env.check_errors()
    for rep in ("turtle", "wide"):
        e = _vec(P3, rep, (7, 7, 7), n, seeds=np.arange(n))
        with pytest.raises(NotImplementedError, match="narrow"):
            e.set_solver_budget(4)
        e.reset()
        e.step(torch.zeros(n, dtype=torch.int32).cuda())  # still synchronous, still working
        e.check_errors()
    e = _vec(P3, "narrow", (7, 7, 7), n, seeds=np.arange(n), controls=["path-length"])
    with pytest.raises(NotImplementedError):
        e.set_solver_budget(4)
    e.check_errors()
    # statistics left stale by pcgrl_update: refused until they are refreshed
    e = _vec(P3, "narrow", (7, 7, 7), n, seeds=np.arange(n))
    e.reset()
    e.update(torch.ones(n, dtype=torch.int32).cuda())
    with pytest.raises(ValueError):
        e.set_solver_budget(4)
    e.refresh_stats()
    e.set_solver_budget(4)
    e.step_ready(act)
    e.check_errors()
    # budget 0 while an env is busy: refused
    g = np.broadcast_to(_serpentine(), (n, 7, 7, 7)).copy()
    e = _vec(P3, "narrow", (7, 7, 7), n, seeds=np.arange(n))
    e.set_solver_budget(1)
    e.reset(init_grids=torch.as_tensor(g))
    assert int(e.env_busy().sum()) == n
    with pytest.raises(ValueError):
        e.set_solver_budget(0)
    e.reset(init_grids=torch.as_tensor(np.ones_like(g)))  # all DIRT: no start candidate, no search, nobody busy
    assert int(e.env_busy().sum()) == 0
    e.set_solver_budget(0)
    e.step(act)
    e.check_errors()


# ------------------------------------------------------------------------------------------------ 9
def test_codes_form_under_step_ready():
    from control_pcgrl_amd.vec_env import codes_to_onehot
    n, budget = 64, 3
    kw = dict(change_percentage=0.05)
    a = _vec(P3, "narrow", (7, 7, 7), n, seeds=np.arange(n), auto_reset=True, obs_format="codes", **kw)
    b = _vec(P3, "narrow", (7, 7, 7), n, seeds=np.arange(n), auto_reset=True, **kw)
    for e in (a, b):
        e.set_solver_budget(budget)
        e.reset()
    g = torch.Generator().manual_seed(2)
    n_emitted = n_busy = 0
    for t in range(150):
        act = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32).cuda()
        oa, ra, da, _, ia = a.step_ready(act)
        ob, rb, db, _, ib = b.step_ready(act)
        assert torch.equal(ia["status"], ib["status"])
        em = (ib["status"] & EMITTED) != 0
        assert oa.shape[1:] == a.obs_shape and oa.shape[-1] == 1
        assert torch.equal(codes_to_onehot(oa, a)[em], ob[em]), t
        assert torch.equal(ia["stats"][em], ib["stats"][em]) and torch.equal(ra[em], rb[em])
        n_emitted += int(em.sum())
        n_busy += int(((ib["status"] & BUSY) != 0).sum())
    assert n_emitted > n and n_busy > 0
    a.check_errors(); b.check_errors()


# ------------------------------------------------------------------------------------------------ 10
def test_seeded_random_sweep_vs_oracle():
    """shapes 3..8 and 9..12 per side, budgets 1..64, batches 1..300, masked resets in between"""
    rng = np.random.default_rng(20261)
    for case in range(10):
        lo, hi = (3, 8) if case % 2 == 0 else (9, 12)
        shape = tuple(int(x) for x in rng.integers(lo, hi + 1, size=3))
        budget = int(rng.integers(1, 65))
        n = int(rng.integers(1, 301)) if case % 2 == 0 else int(rng.integers(1, 41))
        auto_reset = bool(rng.integers(0, 2))
        cp = float(rng.choice([0.02, 0.05, 0.2]))
        seeds = rng.integers(0, 1 << 30, size=n)
        env, orc = _pair(shape, n, auto_reset, seeds=seeds, change_percentage=cp)
        env.set_solver_budget(budget)
        env.reset()
        orc.reset()
        d = Drive(env, orc, n, auto_reset)
        launches = 120 if case % 2 == 0 else 60
        for t in range(launches):
            if t in (launches // 3, 2 * launches // 3):  # a masked reset: abandons the parked steps of the envs it covers
                m = rng.integers(0, 2, size=n).astype(np.uint8)
                env.reset(mask=torch.as_tensor(m))
                orc.reset(mask=m)
                busy = env.env_busy().cpu().numpy().astype(bool)
                d.busy = np.where(m != 0, busy, d.busy)
                d.has_pend[m != 0] = False
                assert np.array_equal(busy, d.busy), "a masked reset does not touch the other envs' flags"
            d.launch(rng.integers(0, 2, size=n).astype(np.int32))
        print(f"case {case}: shape {shape} budget {budget} n {n} auto_reset {auto_reset}: emitted {d.emitted_n.sum()}, "
              f"busy launches {d.busy_launches}")
        assert d.emitted_n.sum() > 0
        d.final_state_equal()
        env.check_errors()
