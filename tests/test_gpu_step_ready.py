"""GPU tests of asynchronous Sokoban stepping (pcgrl_set_solver_budget + pcgrl_step_ready, the resumable solver) against the
CPU oracle: every resumable kernel family, the solver's crate-count limits, checkpoints across solver modes and
refresh_stats while steps are parked.

Protocol (as tests/test_gpu_round6.py _drive_ready): the oracle steps an env exactly when the engine reports EMITTED, with
the action that env consumed; stats / done / observations match bit for bit, rewards to REW_TOL; an env whose status
says it is not busy owes no transition; and after every launch pcgrl_env_busy equals the status's BUSY bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pcgrl_oracle as po  # noqa: E402  (checker only)
from conftest import GOLDEN  # noqa: E402

REW_TOL = 1e-6


def _vec(*a, **k):
    from control_pcgrl_amd import VecPcgrlEnv
    return VecPcgrlEnv(*a, **k)


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------- playable levels + a policy
def rooms(n, shape, seed, rep, k_max=3, room=None):
    """sokoban levels that meet the solver's precondition (one player, k crates = k targets, one region): one room carved
    into solid (bench.solver_active_maps for any H x W).  Returns (maps uint8 [n, H, W], boxes int [n, 4] = y0, x0, h, w,
    init_pos int32 [n, 2] on a floor cell of the room).  narrow walks the map in row-major order after its first edit:
    its rooms start in the top-left corner, so that the walk crosses them at once."""
    H, W = shape
    rng = np.random.default_rng(seed)
    g = np.ones((n, H, W), np.uint8)
    boxes = np.zeros((n, 4), np.int64)
    pos = np.zeros((n, 2), np.int32)
    for i in range(n):
        if room is not None:
            h, w = room
        else:
            h = int(rng.integers(3, min(6, H - 2) + 1))
            w = int(rng.integers(3, min(8 if rep != "narrow" else 14, W - 2) + 1))
        if rep == "narrow":
            y0, x0 = 0, 0
        else:
            y0, x0 = int(rng.integers(1, H - h)), int(rng.integers(1, W - w))
        g[i, y0:y0 + h, x0:x0 + w] = 0
        k = min(int(rng.integers(1, k_max + 1)), (h * w - 2) // 2)
        pick = rng.permutation(h * w)[:2 + 2 * k]
        for c, t in zip(pick[:1 + 2 * k], [2] + [3] * k + [4] * k):
            g[i, y0 + c // w, x0 + c % w] = t
        pos[i] = (y0 + pick[-1] // w, x0 + pick[-1] % w)  # (a floor cell)
        boxes[i] = (y0, x0, h, w)
    return g, boxes, pos


def _editable(boxes, shape):
    """[n, H, W] bool: the room and its 4-neighbourhood (no corners), where the policy may put floor or wall"""
    H, W = shape
    n = len(boxes)
    m = np.zeros((n, H, W), bool)
    for i, (y0, x0, h, w) in enumerate(boxes):
        m[i, max(y0 - 1, 0):y0 + h + 1, x0:x0 + w] = True
        m[i, y0:y0 + h, max(x0 - 1, 0):x0 + w + 1] = True
    return m


class Policy:
    """floor / wall edits inside the room (never on the player, a crate or a target), chosen from the oracle's state --
    which is the engine's committed state for every env that is about to consume an action"""

    def __init__(self, rep, shape, boxes, seed, p_edit=0.6):
        self.rep, self.shape, self.boxes = rep, shape, np.asarray(boxes)
        self.ed = _editable(self.boxes, shape)
        self.rng = np.random.default_rng(seed)
        self.p_edit = p_edit

    def __call__(self, orc):
        H, W = self.shape
        s = orc.get_state()
        g = s["grids"].reshape(-1, H, W)
        n = len(g)
        r, c = s["pos"][:, 0], s["pos"][:, 1]
        i = np.arange(n)
        tile = g[i, r, c].astype(np.int32)
        ok = self.ed[i, r, c] & (tile <= 1)
        pick = self.rng.integers(0, 2, n).astype(np.int32)
        edit = ok & (self.rng.random(n) < self.p_edit)
        if self.rep == "narrow":  # Discrete(n_tiles) at the walk's position: keep the tile outside the room
            return np.where(edit, pick, tile).astype(np.int32)
        if self.rep == "turtle":  # 4 moves (up, down, left, right) + 4 + tile
            y0, x0, h, w = self.boxes.T
            a = np.empty(n, np.int32)
            for j in range(n):
                if edit[j]:
                    a[j] = 4 + pick[j]
                    continue
                dirs = [d for d, (dy, dx) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1)))
                        if y0[j] <= r[j] + dy < y0[j] + h[j] and x0[j] <= c[j] + dx < x0[j] + w[j]]
                a[j] = self.rng.choice(dirs) if dirs else 4 + tile[j]
            return a
        # wide: ActionMap's (column, row, tile) index (wide_rep.py:40-45), a random editable floor / wall cell
        a = np.empty(n, np.int32)
        for j in range(n):
            cells = np.argwhere(self.ed[j] & (g[j] <= 1))
            if len(cells) == 0:
                a[j] = int(g[j, 0, 0])  # (cell (0, 0), its own tile: no change)
                continue
            y, x = cells[self.rng.integers(0, len(cells))]
            t = int(pick[j]) if self.rng.random() < self.p_edit else int(g[j, y, x])
            a[j] = (x * H + y) * 5 + t
        return a


# ------------------------------------------------------------------------------------- the ready protocol
class Ready:
    """an engine with a solver budget and its oracle, driven under the ready protocol"""

    def __init__(self, env, orc, auto_reset, check_obs_every=1):
        self.env, self.orc, self.auto = env, orc, bool(auto_reset)
        self.n = env.num_envs
        self.check_obs_every = check_obs_every
        self.pend = np.zeros(self.n, np.int32)
        self.has_pend = np.zeros(self.n, bool)
        self.busy = _np(env.env_busy()).astype(bool)
        self.t = self.emitted = self.busy_launches = self.max_streak = 0
        self.streak = np.zeros(self.n, int)
        self.log = []  # per launch: (emitted mask, actions the oracle played) -- replays the oracle's trajectory

    def snapshot(self):
        return self.busy.copy(), self.pend.copy(), self.has_pend.copy()

    def restore(self, snap):
        self.busy, self.pend, self.has_pend = (a.copy() for a in snap)

    def reset(self, mask=None, init_grids=None, init_pos=None):
        """a reset (abandons the steps in flight of the envs it covers: the oracle never played them)"""
        m = None if mask is None else torch.as_tensor(mask, dtype=torch.uint8)
        g = None if init_grids is None else torch.as_tensor(init_grids)
        p = None if init_pos is None else torch.as_tensor(init_pos, dtype=torch.int32)
        self.env.reset(mask=m, init_grids=g, init_pos=p)
        self.orc.reset(mask=mask, init_grids=init_grids, init_pos=init_pos)
        self.has_pend[np.ones(self.n, bool) if mask is None else np.asarray(mask, bool)] = False
        self.busy = _np(self.env.env_busy()).astype(bool)

    def launch(self, a):
        env, orc, t = self.env, self.orc, self.t
        consume = ~self.busy
        self.pend[consume] = a[consume]
        self.has_pend[consume] = True
        obs, rew, done, _, info = env.step_ready(torch.as_tensor(a, dtype=torch.int32).to(env.device))
        status = _np(info["status"])
        emitted = (status & 1) != 0
        assert not (emitted & ~self.has_pend).any(), f"launch {t}: a transition without a consumed action"
        oobs, orew, odone, ostats = orc.step_masked(emitted, self.pend, auto_reset=self.auto)
        self.log.append((emitted.copy(), self.pend.copy()))
        if emitted.any():
            st = _np(info["stats"])
            bad = emitted & (st != ostats).any(axis=1)
            assert not bad.any(), f"launch {t}: env {int(np.argmax(bad))} stats {st[bad][0].tolist()} != {ostats[bad][0].tolist()}"
            assert np.abs(_np(rew)[emitted] - orew[emitted]).max() <= REW_TOL, t
            assert np.array_equal(_np(done)[emitted], odone[emitted]), t
            if t % self.check_obs_every == 0:
                assert np.array_equal(_np(obs)[emitted], oobs[emitted]), t
        self.has_pend[emitted] = False
        self.busy = (status & 2) != 0
        assert np.array_equal(_np(env.env_busy()).astype(bool), self.busy), f"launch {t}: pcgrl_env_busy != the status's BUSY bit"
        assert not (~self.busy & self.has_pend).any(), f"launch {t}: an idle env still owes a transition"
        self.emitted += int(emitted.sum())
        self.busy_launches += int(self.busy.any())
        self.streak = np.where(self.busy, self.streak + 1, 0)
        self.max_streak = max(self.max_streak, int(self.streak.max()))
        self.t += 1
        return status

    def finish(self):
        """grids, the idle envs' statistics and the last-episode totals against the oracle; no error was raised"""
        env, orc, n = self.env, self.orc, self.n
        idle = ~_np(env.env_busy()).astype(bool)
        st, ost = env.get_state(), orc.get_state()
        assert np.array_equal(_np(st.grids).reshape(n, -1), ost["grids"])
        assert np.array_equal(_np(st.stats)[idle], ost["stats"][idle])
        le, ole = env.last_episode(), orc.last_episode()
        assert np.array_equal(_np(le.n_episodes), ole["n_episodes"])
        assert np.array_equal(_np(le.final_stats), ole["final_stats"])
        env.check_errors()


def _pair(rep, shape, n, seed, auto_reset, budget=None, **kw):
    seeds = seed + np.arange(n)
    env = _vec("sokoban", rep, shape, n, seeds=seeds, auto_reset=auto_reset, **kw)
    orc = po.OracleVecEnv("sokoban", rep, shape, n, seeds=seeds, **kw)
    if budget:
        env.set_solver_budget(budget)
    return env, orc


def _noop(rep, shape, orc):
    """actions that change no map (a narrow / wide write of the tile already there, a turtle write at its position)"""
    H, W = shape
    s = orc.get_state()
    g = s["grids"].reshape(-1, H, W)
    i = np.arange(len(g))
    r, c = s["pos"][:, 0], s["pos"][:, 1]
    tile = g[i, r, c].astype(np.int32)
    if rep == "narrow":
        return tile
    if rep == "turtle":
        return 4 + tile
    return g[:, 0, 0].astype(np.int32)  # (wide: cell (0, 0), its own tile)


def _drain(d, rep, shape, budget=4):
    """launches of actions that start no search until no env is busy: one launch with a budget no search exceeds (the
    budget decides in which launch a search ends, never its result), then the small budget again"""
    d.env.set_solver_budget(1 << 20)
    d.launch(_noop(rep, shape, d.orc))
    assert not d.busy.any()
    d.env.set_solver_budget(budget)


# ------------------------------------------------------------------------------------- A. every resumable kernel family
# (family = lanes per env + row-mask type, fixed by the shape: pcgrl_engine.hip validate(); "fast" = the compile-time 16x16
# kernel, which the default window / wide at 16x16 selects)
FAMILIES = [
    ("l16-u32-fast", "narrow", (16, 16), None, 8, False),
    ("l16-u32-fast", "turtle", (16, 16), None, 16, True),
    ("l16-u32-general", "narrow", (16, 16), (15, 9), 6, True),
    ("l16-u32-general", "wide", (12, 12), None, 12, False),
    ("l8-u32", "narrow", (8, 20), None, 4, True),
    ("l32-u32", "narrow", (20, 20), None, 10, False),
    ("l32-u32", "turtle", (32, 32), None, 24, True),
    ("l64-u32", "narrow", (48, 20), None, 8, True),
    ("l64-u32", "narrow", (62, 32), None, 16, False),
    ("l32-u64", "narrow", (20, 40), None, 12, True),
    ("l64-u64", "wide", (40, 40), None, 20, False),
    ("l64-u64", "narrow", (62, 62), None, 6, True),
]


@pytest.mark.parametrize("family,rep,shape,window,budget,auto", FAMILIES,
                         ids=[f"{f[0]}-{f[1]}-{f[2][0]}x{f[2][1]}" + (f"-win{f[3][0]}x{f[3][1]}" if f[3] else "") for f in FAMILIES])
def test_step_ready_kernel_family_vs_oracle(family, rep, shape, window, budget, auto):
    """playable levels, small budgets: searches park over several launches, busy envs ignore their actions, re-injected
    levels abandon steps in flight; every emitted transition equals the oracle's"""
    n, steps = 48, 150
    kw = dict(solver_power=200)
    if window is not None:
        kw["obs_window"] = window
    if auto:
        kw["change_percentage"] = 0.05  # episodes end within the run: auto-resets while searches are parked elsewhere
    env, orc = _pair(rep, shape, n, 11 + budget, auto, budget, **kw)
    maps, boxes, pos = rooms(n, shape, budget, rep)
    pol = Policy(rep, shape, boxes, budget)
    d = Ready(env, orc, auto, check_obs_every=1 if shape[0] * shape[1] <= 1024 else 3)
    d.reset(init_grids=maps, init_pos=pos)
    for t in range(steps):
        if auto and t % 50 == 49:
            d.reset(mask=(np.arange(n) % 2 == t % 2).astype(np.uint8), init_grids=maps, init_pos=pos)
        d.launch(pol(orc))
    # it searched: a case in which nothing parked proves nothing
    assert d.emitted > n and d.busy_launches >= 10 and d.max_streak >= 3, (d.emitted, d.busy_launches, d.max_streak)
    d.finish()


# ------------------------------------------------------------------------------------- B. crate-count limits
def _crowded(n, shape, k_lo, k_hi, seed):
    """levels with k_lo..k_hi crates in one room: crates on a checkerboard of its interior (no 2x2 blocks, none against
    the room's walls), targets and the player on the other cells"""
    H, W = shape
    rng = np.random.default_rng(seed)
    g = np.ones((n, H, W), np.uint8)
    boxes = np.zeros((n, 4), np.int64)
    y0, x0, h, w = 1, 1, H - 2, W - 2
    ys, xs = np.mgrid[y0 + 1:y0 + h - 1, x0 + 1:x0 + w - 1]
    checker = [(y, x) for y, x in zip(ys.ravel(), xs.ravel()) if (y + x) % 2 == 0]
    for i in range(n):
        g[i, y0:y0 + h, x0:x0 + w] = 0
        k = int(rng.integers(k_lo, k_hi + 1))
        assert k <= len(checker)
        for j in rng.permutation(len(checker))[:k]:
            g[i, checker[j][0], checker[j][1]] = 3
        free = np.argwhere(g[i] == 0)
        sel = free[rng.permutation(len(free))[:k + 1]]
        g[i, sel[0][0], sel[0][1]] = 2
        for y, x in sel[1:]:
            g[i, y, x] = 4
        boxes[i] = (y0, x0, h, w)
    return g, boxes


def test_step_ready_two_register_crate_lists_vs_oracle():
    """NH = 2 (65..128 crates): the resumable solver's two-register crate lists, parked and resumed several times"""
    n, shape, steps = 16, (24, 24), 100
    env, orc = _pair("wide", shape, n, 5, False, 8, solver_power=60)
    maps, boxes = _crowded(n, shape, 66, 100, 2)
    st = po.stats_for_grids("sokoban", maps, solver_power=60)
    assert ((st[:, 1] > 64) & (st[:, 1] <= 128) & (st[:, 1] == st[:, 2]) & (st[:, 3] == 1) & (st[:, 0] == 1)).all()
    pol = Policy("wide", shape, boxes, 3)
    d = Ready(env, orc, False)
    d.reset(init_grids=maps)
    for _ in range(steps):
        d.launch(pol(orc))
    assert d.emitted >= n and d.busy_launches >= 20 and d.max_streak >= 3, (d.emitted, d.busy_launches, d.max_streak)
    d.finish()


def test_step_ready_more_than_128_pairs_golden():
    """levels with 129 .. 505 pairs (the reference's answers) loaded while a budget is set: their statistics are the
    synchronous solver's, not the solver-less ones, and no limit is reported"""
    z = np.load(f"{GOLDEN}/stats_sokoban_solver_huge.npz")
    for g, want, power, shape in zip(z["grids"], z["stats"], z["solver_power"], z["shapes"]):
        h, w = int(shape[0]), int(shape[1])
        grid = np.ascontiguousarray(g[:h, :w])
        n = 3
        env = _vec("sokoban", "narrow", (h, w), n, auto_reset=False, solver_power=int(power))
        orc = po.OracleVecEnv("sokoban", "narrow", (h, w), n, solver_power=int(power))
        env.set_solver_budget(8)
        d = Ready(env, orc, False)
        d.reset(init_grids=np.repeat(grid[None], n, 0))
        for _ in range(64):
            if not d.busy.any():
                break
            d.launch(_noop("narrow", (h, w), orc))
        assert not d.busy.any()
        st = _np(env.get_state().stats)
        assert np.array_equal(st, np.repeat(want[None], n, 0)), f"{h}x{w} power {int(power)}: {st.tolist()} want {want.tolist()}"
        env.check_errors()
        env.close()


def test_step_ready_more_than_128_pairs_vs_oracle():
    """a 140-pair level (reference answer in the fixture) edited under a budget, next to small parked searches: every
    emitted transition equals the oracle's"""
    z = np.load(f"{GOLDEN}/stats_sokoban_solver_huge.npz")
    i = [j for j, s in enumerate(z["shapes"]) if tuple(s) == (24, 21)][0]
    h, w = 24, 21
    big = np.ascontiguousarray(z["grids"][i][:h, :w])
    n = 16
    env, orc = _pair("narrow", (h, w), n, 9, False, 6, solver_power=int(z["solver_power"][i]))
    small, boxes, pos = rooms(n, (h, w), 4, "narrow")
    maps = small.copy()
    maps[::2] = big  # even envs: the huge level (edits anywhere in it), odd envs: rooms with resumable searches
    boxes[::2] = (0, 0, h, w)
    pos[::2] = np.argwhere(big == 0)[0]
    pol = Policy("narrow", (h, w), boxes, 6)
    d = Ready(env, orc, False)
    d.reset(init_grids=maps, init_pos=pos)
    assert not d.busy[::2].any(), "a level over 128 pairs is searched to the end within the launch"
    assert np.array_equal(_np(env.get_state().stats)[::2], np.repeat(z["stats"][i][None], n // 2, 0))
    for _ in range(120):
        d.launch(pol(orc))
    assert d.busy_launches >= 5, d.busy_launches
    d.finish()


# ------------------------------------------------------------------------------------- C. checkpoints across solver modes
def _busy_budgeted(n=24, shape=(20, 20), budget=4, seed=21, steps=40):
    env, orc = _pair("narrow", shape, n, seed, False, budget, solver_power=300)
    maps, boxes, pos = rooms(n, shape, seed, "narrow")
    pol = Policy("narrow", shape, boxes, seed)
    d = Ready(env, orc, False)
    d.reset(init_grids=maps, init_pos=pos)
    for _ in range(steps):
        d.launch(pol(orc))
    for _ in range(200):  # until a launch leaves some env busy
        if d.busy.any():
            break
        d.launch(pol(orc))
    assert d.busy.any() and (~d.busy).any()
    return d, pol, maps, pos, boxes


def test_budgeted_checkpoint_with_busy_envs_refused_by_synchronous_engine():
    """an image with busy envs into an engine without a budget: refused (full, or masked over a busy env) before anything
    is overwritten, the engine goes on bit-exactly; a mask of idle envs only is accepted"""
    d, pol, maps, pos, boxes = _busy_budgeted()
    n, shape = d.n, (20, 20)
    sd = d.env.state_dict()
    sync, sorc = _pair("narrow", shape, n, 77, False, None, solver_power=300)
    sync.reset(init_grids=torch.as_tensor(maps), init_pos=torch.as_tensor(pos))
    sorc.reset(init_grids=maps, init_pos=pos)
    before = _np(sync.state_dict()["blob"])
    with pytest.raises(ValueError):
        sync.load_state_dict(sd)
    with pytest.raises(ValueError):  # a mask that covers one busy env
        sync.load_state_dict(sd, mask=(np.arange(n) == int(np.argmax(d.busy))).astype(np.uint8))
    assert np.array_equal(_np(sync.state_dict()["blob"]), before), "a refused import overwrote something"
    spol = Policy("narrow", shape, boxes, 5)
    for t in range(30):  # the synchronous engine goes on bit-exactly
        a = spol(sorc)
        _, rew, done, _, info = sync.step(torch.as_tensor(a).cuda())
        _, orew, odone, ostats = sorc.step(a)
        assert np.array_equal(_np(info["stats"]), ostats) and np.abs(_np(rew) - orew).max() <= REW_TOL, t
        assert np.array_equal(_np(done), odone), t
    sync.check_errors()
    # a mask of idle envs only is accepted: those rows are the budgeted engine's
    idle = (~d.busy).astype(np.uint8)
    sync.load_state_dict(sd, mask=idle)
    a, b = sync.get_state(), d.env.get_state()
    assert np.array_equal(_np(a.grids)[idle == 1], _np(b.grids)[idle == 1])
    assert np.array_equal(_np(a.stats)[idle == 1], _np(b.stats)[idle == 1])
    assert np.array_equal(_np(a.grids)[idle == 0].reshape(-1, 400), sorc.get_state()["grids"][idle == 0])
    sync.check_errors()
    # ... and the budgeted engine itself goes on
    for _ in range(20):
        d.launch(pol(d.orc))
    d.finish()


def test_stale_checkpoint_refused_by_budgeted_engine():
    """an image that may carry statistics left stale by update() into an engine with a budget: refused"""
    n, shape = 16, (16, 16)
    sync, _ = _pair("wide", shape, n, 3, False, None, solver_power=200)
    sync.reset()
    sync.update(torch.zeros(n, dtype=torch.int32).cuda())  # statistics go stale
    sd = sync.state_dict()
    assert sd["maybe_stale"] == 1
    bud, _ = _pair("wide", shape, n, 3, False, 8, solver_power=200)
    bud.reset()
    before = _np(bud.state_dict()["blob"])
    with pytest.raises(ValueError):
        bud.load_state_dict(sd)
    with pytest.raises(ValueError):
        bud.load_state_dict(sd, mask=np.ones(n, np.uint8))
    assert np.array_equal(_np(bud.state_dict()["blob"]), before)
    with pytest.raises(ValueError):  # the same rule as pcgrl_set_solver_budget's
        sync.set_solver_budget(8)


def test_synchronous_checkpoint_continues_in_budgeted_engine():
    """a synchronous engine's checkpoint goes on under a budget, against the oracle that played the synchronous steps"""
    n, shape = 32, (20, 20)
    sync, orc = _pair("narrow", shape, n, 31, True, None, solver_power=300, change_percentage=0.05)
    maps, boxes, pos = rooms(n, shape, 31, "narrow")
    pol = Policy("narrow", shape, boxes, 31)
    sync.reset(init_grids=torch.as_tensor(maps), init_pos=torch.as_tensor(pos))
    orc.reset(init_grids=maps, init_pos=pos)
    for t in range(25):
        a = pol(orc)
        _, _, _, _, info = sync.step(torch.as_tensor(a).cuda())
        assert np.array_equal(_np(info["stats"]), orc.step(a, auto_reset=True)[3]), t
    sd = sync.state_dict()
    bud, _ = _pair("narrow", shape, n, 999, True, 4, solver_power=300, change_percentage=0.05)
    bud.load_state_dict(sd)
    d = Ready(bud, orc, True)
    for _ in range(80):
        d.launch(pol(orc))
    assert d.busy_launches >= 5, d.busy_launches
    d.finish()


def test_idle_budgeted_checkpoint_continues_in_synchronous_engine():
    """train asynchronously, evaluate synchronously: a checkpoint taken when no env is busy"""
    d, pol, maps, pos, _ = _busy_budgeted(seed=41)
    _drain(d, "narrow", (20, 20))
    sd = d.env.state_dict()
    sync, _ = _pair("narrow", (20, 20), d.n, 5, False, None, solver_power=300)
    sync.load_state_dict(sd)
    orc = d.orc
    for t in range(40):
        a = pol(orc)
        obs, rew, done, _, info = sync.step(torch.as_tensor(a).cuda())
        oobs, orew, odone, ostats = orc.step(a)
        assert np.array_equal(_np(info["stats"]), ostats) and np.abs(_np(rew) - orew).max() <= REW_TOL, t
        assert np.array_equal(_np(done), odone) and np.array_equal(_np(obs), oobs), t
    sync.check_errors()


def test_older_budgeted_checkpoint_back_into_the_same_engine():
    """park records that belong to later levels / searches further along than the image's: results never depend on them"""
    d, pol, maps, pos, _ = _busy_budgeted(seed=51, steps=30)
    sd, snap, k = d.env.state_dict(), d.snapshot(), d.t
    for _ in range(60):
        d.launch(pol(d.orc))
    d.env.load_state_dict(sd)
    # a fresh oracle replays the recorded launches up to the checkpoint
    orc = po.OracleVecEnv("sokoban", "narrow", (20, 20), d.n, seeds=51 + np.arange(d.n), solver_power=300)
    orc.reset(init_grids=maps, init_pos=pos)
    for emitted, acts in d.log[:k]:
        orc.step_masked(emitted, acts, auto_reset=False)
    d.orc = orc
    d.restore(snap)
    assert np.array_equal(_np(d.env.env_busy()).astype(bool), d.busy)
    for _ in range(80):
        d.launch(pol(orc))
    assert d.busy_launches >= 5
    d.finish()


def test_portable_state_under_budget_equals_oracle_reset():
    """load_state_dict in the portable form (pcgrl_set_state, counters zero) with a budget set == the oracle's
    reset(init_grids=...), including the envs it leaves busy"""
    n, shape = 32, (20, 40)
    env, orc = _pair("narrow", shape, n, 61, False, 4, solver_power=400)
    maps, boxes, pos = rooms(n, shape, 61, "narrow", k_max=4)
    sd = {"grids": maps, "pos": np.concatenate([pos, np.zeros((n, 1), np.int32)], 1), "counters": np.zeros((n, 4), np.int32),
          "ep_return": np.zeros(n), "rng": env.get_rng_state()}
    env.load_state_dict(sd)
    orc.reset(init_grids=maps, init_pos=pos)
    d = Ready(env, orc, False)
    assert d.busy.any(), "some level's search outlasts the budget"
    _drain(d, "narrow", shape)
    st, ost = env.get_state(), orc.get_state()
    assert np.array_equal(_np(st.stats), ost["stats"]) and np.array_equal(_np(st.last_loss), ost["last_loss"])
    pol = Policy("narrow", shape, boxes, 62)
    for _ in range(40):
        d.launch(pol(orc))
    d.finish()


# ------------------------------------------------------------------------------------- D. refresh_stats while parked
def test_refresh_stats_while_steps_are_parked():
    """refresh_stats in launches where some env has a parked step: a status of 0 still means idle, and the next action is
    consumed; the refreshed rows of idle envs and of envs with a parked step hold the statistics of their current maps"""
    n, shape = 32, (16, 16)
    env, orc = _pair("turtle", shape, n, 71, False, 2, solver_power=1000)
    maps, boxes, pos = rooms(n, shape, 71, "turtle", k_max=3)
    pol = Policy("turtle", shape, boxes, 72, p_edit=0.8)
    d = Ready(env, orc, False)
    d.reset(init_grids=maps, init_pos=pos)
    refreshed = 0
    for t in range(160):
        d.launch(pol(orc))
        parked = d.busy & d.has_pend
        if parked.any() and t % 3 == 0:
            got = _np(env.refresh_stats())
            ost = orc.get_state()["stats"]
            busy = _np(env.env_busy()).astype(bool)
            rows = ~busy | parked
            assert np.array_equal(got[rows], ost[rows]), t
            d.busy = busy
            refreshed += 1
    assert refreshed >= 5, refreshed
    d.finish()
