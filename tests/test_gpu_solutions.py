"""Sokoban solutions (include/pcgrl_amd_solutions.h) on the GPU: every fixture recorded from the reference
(tests/golden/solutions/, tools/gen_golden_solutions.py, and the solver fixtures tests/golden/stats_sokoban*.npz) and fresh
small-room levels against the plain-Python rules (tests/sokoban_rules.py), move for move; the engine's own maps after resets /
steps / updates / restores on every kernel form; caps between guard bytes; a solver budget with searches parked; steps with a
solutions call in between against the CPU oracle; graph capture; sub-batching, the gym adapter and the refusals.

The kernel states the solver's loop a second time (csrc/solutions/pcgrl_solutions.h sol_stage next to pcgrl_sokoban.h sk_stage):
every test here that touches a level also compares `length` / `dist_win` with the statistics (sol-length, dist-win) the step and
statistics kernels compute for it."""
import glob
import os

import numpy as np
import pytest

import sokoban_rules as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from conftest import GOLDEN  # noqa: E402
from test_gpu_step_ready import Policy, Ready, _pair, rooms  # noqa: E402  (playable levels, the ready protocol)

SOL = os.path.join(GOLDEN, "solutions")
ROOMS = sorted(glob.glob(os.path.join(SOL, "rooms_*.npz")))
DIST_WIN, SOL_LENGTH = 4, 5  # columns of the sokoban statistics


def _vec(*a, **k):
    from control_pcgrl_amd import VecPcgrlEnv
    return VecPcgrlEnv(*a, **k)


def _np(t):
    return t.cpu().numpy()


def _shape_of(path):
    return tuple(int(v) for v in os.path.basename(path)[6:-4].split("x"))


def _room_file(path):
    """-> (grids, move lists, length, dist_win)"""
    z = np.load(path)
    off = z["offsets"]
    return z["grids"], [z["moves"][off[i]:off[i + 1]].tolist() for i in range(len(z["grids"]))], z["length"], z["dist_win"]


def _as_array(sols, cap):
    """move lists -> int8 [n, cap], -1 behind each list"""
    out = np.full((len(sols), cap), -1, np.int8)
    for i, s in enumerate(sols):
        out[i, :min(len(s), cap)] = s[:cap]
    return out


def _check(out, sols, length, dist_win, what):
    """a solutions() result against move lists (None: not known), lengths and dist-win values"""
    cap = out.moves.shape[1]
    assert out.moves.dtype == torch.int8 and out.length.dtype == torch.int32 and out.dist_win.dtype == torch.int32
    got_len, got_dw, got = _np(out.length), _np(out.dist_win), _np(out.moves)
    bad = np.flatnonzero(got_len != length)
    assert bad.size == 0, f"{what}: length differs in {bad.size} maps, first {bad[:5]}: {got_len[bad[:5]]} != {np.asarray(length)[bad[:5]]}"
    bad = np.flatnonzero(got_dw != dist_win)
    assert bad.size == 0, f"{what}: dist_win differs in {bad.size} maps, first {bad[:5]}: {got_dw[bad[:5]]} != {np.asarray(dist_win)[bad[:5]]}"
    for i, s in enumerate(sols):
        n = max(int(length[i]), 0)
        assert (got[i, min(n, cap):] == -1).all(), f"{what}: map {i}: bytes behind the solution"
        if s is not None:
            assert got[i, :min(n, cap)].tolist() == list(s[:cap]), f"{what}: map {i}: {got[i, :n].tolist()} != {s}"


def _consistent(env, out, grids, what):
    """the properties that hold for ANY maps: `length` / `dist_win` are the statistics kernels' sol-length / dist-win, and every
    solved map's moves replay to a win.  -> number of solved maps"""
    st = _np(env.stats_for_grids(grids))
    need = (st[:, 0] == 1) & (st[:, 1] == st[:, 2]) & (st[:, 1] > 0) & (st[:, 3] == 1)
    length, moves = _np(out.length), _np(out.moves)
    assert np.array_equal(length, np.where(need, st[:, SOL_LENGTH], -1)), what
    assert np.array_equal(np.maximum(length, 0), st[:, SOL_LENGTH]), what
    assert np.array_equal(_np(out.dist_win), st[:, DIST_WIN]), what
    g = _np(grids).reshape((len(length),) + env.map_shape)
    for i in np.flatnonzero(length > 0):
        assert sr.replay(g[i], moves[i, :length[i]]) == (True, True), f"{what}: env {i}"
    assert (moves[np.arange(moves.shape[1])[None, :] >= np.maximum(length, 0)[:, None]] == -1).all(), what
    return int((length > 0).sum())


# ---- the fixtures through solutions_for_grids ---------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ROOMS, ids=[os.path.basename(f)[:-4] for f in ROOMS])
def test_room_fixtures_through_solutions_for_grids(path):
    grids, sols, length, dist_win = _room_file(path)
    shape = _shape_of(path)
    env = _vec("sokoban", "narrow", shape, 4)
    assert env._L.pcgrl_solution_capacity(env._h) == 10000
    # the whole file in one call; then counts that are no multiple of anything
    for n in (len(grids), 7, 1):
        out = env.solutions_for_grids(torch.as_tensor(grids[:n]), dist_win=True)
        assert tuple(out.moves.shape) == (n, 10000)
        _check(out, sols[:n], length[:n], dist_win[:n], f"{os.path.basename(path)} n={n}")
    out = env.solutions_for_grids(torch.as_tensor(grids), cap=128, dist_win=True)
    assert _consistent(env, out, torch.as_tensor(grids).to(env.device), path) == int((length > 0).sum())
    assert env.solutions_for_grids(torch.as_tensor(grids), cap=5).dist_win is None
    env.check_errors()
    env.close()


def _stats_arrays():
    """(id, grids, stats, {index: moves}) of every committed solver fixture answered with the default solver_power"""
    z = np.load(os.path.join(SOL, "fixture_solutions.npz"))
    known = {}
    for k, (src, i) in enumerate(zip(z["source"], z["index"])):
        known.setdefault(str(src), {})[int(i)] = z["moves"][z["offsets"][k]:z["offsets"][k + 1]].tolist()
    out = []
    for fname in ("stats_sokoban.npz", "stats_sokoban_solver.npz", "stats_sokoban_solver_shapes.npz", "stats_sokoban_solver_wide.npz"):
        f = np.load(os.path.join(GOLDEN, fname))
        for key in f.files:
            if key.startswith("grids"):
                out.append((f"{fname[:-4]}{key[5:]}", f[key], f[key.replace("grids", "stats")], known.get(f"{fname}:{key}", {})))
    return out


STATS_ARRAYS = _stats_arrays()


@pytest.mark.parametrize("name,grids,stats,known", STATS_ARRAYS, ids=[a[0] for a in STATS_ARRAYS])
def test_solver_fixtures_through_solutions_for_grids(name, grids, stats, known):
    """every level of the solver fixtures: the recorded solution where the stored sol-length is > 0, length 0 / -1 as the stored
    statistics say elsewhere (dense levels of up to 127 pairs that run every stage to its cap among them)"""
    need = (stats[:, 0] == 1) & (stats[:, 1] == stats[:, 2]) & (stats[:, 1] > 0) & (stats[:, 3] == 1)
    length = np.where(need, stats[:, SOL_LENGTH], -1)
    assert set(known) == set(np.flatnonzero(length > 0).tolist())
    sols = [known.get(i, []) for i in range(len(grids))]
    env = _vec("sokoban", "narrow", grids.shape[1:], 4)
    for n in (len(grids), 5):
        out = env.solutions_for_grids(torch.as_tensor(grids[:n]), cap=64, dist_win=True)
        _check(out, sols[:n], length[:n], stats[:n, DIST_WIN], f"{name} n={n}")
    for i, s in known.items():
        assert sr.replay(grids[i], s) == (True, True)
    env.check_errors()
    env.close()


def test_levels_of_more_than_128_pairs():
    """the eight-register form (129 .. 505 pairs; none of the known levels is solved): length 0 / -1 and dist_win as the stored
    statistics say, each level with the shape and solver_power it was answered with, and no error bit"""
    z = np.load(os.path.join(GOLDEN, "stats_sokoban_solver_huge.npz"))
    for g, st, power, (h, w) in zip(z["grids"], z["stats"], z["solver_power"], z["shapes"]):
        env = _vec("sokoban", "narrow", (int(h), int(w)), 2, solver_power=int(power))
        assert env._L.pcgrl_solution_capacity(env._h) == int(power)
        grid = torch.as_tensor(np.ascontiguousarray(g[None, :h, :w]))
        out = env.solutions_for_grids(grid, cap=8, dist_win=True)
        need = st[0] == 1 and st[1] == st[2] and st[1] > 128 and st[3] == 1
        assert need and st[SOL_LENGTH] == 0
        _check(out, [[]], [0], [st[DIST_WIN]], f"{h}x{w} {st[1]} pairs")
        assert np.array_equal(_np(env.stats_for_grids(grid))[0], st)
        env.check_errors()  # (no level beyond the solver's limits)
        env.close()


# ---- fresh levels against the plain-Python rules ------------------------------------------------------------------------------
_FRESH = {}


def _fresh(shape, n, seed):
    """n small-room levels and their answers by the plain-Python rules (computed once)"""
    if (shape, n) not in _FRESH:
        rng = np.random.default_rng(seed)
        grids = np.array([sr.small_room(rng, shape, x_from=26 if shape[1] > 32 and i % 2 else None) for i in range(n)], np.uint8)
        ans = [sr.solve(g, 10000) if sr.precondition(g) else None for g in grids]
        _FRESH[(shape, n)] = (grids, ans)
    return _FRESH[(shape, n)]


@pytest.mark.parametrize("shape,n", [((16, 16), 200), ((20, 40), 40)], ids=["16x16", "20x40"])
def test_fresh_small_rooms_against_the_python_rules(shape, n):
    grids, ans = _fresh(shape, n, 20261017 + shape[1])
    sols = [a[0] if a else [] for a in ans]
    length = np.array([len(a[0]) if a else -1 for a in ans])
    dist_win = np.array([a[1] if a else shape[0] * shape[1] * sum(shape) for a in ans])
    assert (length > 0).sum() >= n // 10  # (about one level in five of this family is solved)
    env = _vec("sokoban", "narrow", shape, 4)
    out = env.solutions_for_grids(torch.as_tensor(grids), cap=256, dist_win=True)
    _check(out, sols, length, dist_win, f"fresh {shape}")
    _consistent(env, out, torch.as_tensor(grids).to(env.device), f"fresh {shape}")
    env.check_errors()
    env.close()


# ---- the engine's own maps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ROOMS, ids=[os.path.basename(f)[:-4] for f in ROOMS])
def test_own_maps_on_every_form(path):
    """solutions() reads the engine's tile planes, solutions_for_grids the bytes get_state() hands out: the two agree -- and
    agree with the statistics -- after a reset with injected levels, after steps, after update() without refresh_stats(), after
    a masked reset and after load_state_dict.  The eight shapes cover the six (lanes per map, mask width) forms."""
    grids, sols, length, dist_win = _room_file(path)
    shape, n, steps = _shape_of(path), len(grids), 3
    env = _vec("sokoban", "narrow", shape, n, seeds=3 + np.arange(n), auto_reset=False)
    env.reset(init_grids=grids, init_pos=np.zeros((n, 2), np.int32))

    def check(what):
        own = env.solutions(cap=128, dist_win=True)
        g = env.get_state().grids
        other = env.solutions_for_grids(g, cap=128, dist_win=True)
        for key in ("moves", "length", "dist_win"):
            assert torch.equal(getattr(own, key), getattr(other, key)), f"{path} {what}: {key}"
        return own, g, _consistent(env, own, g, f"{path} {what}")

    own, g, _ = check("after reset")
    _check(own, sols, length, dist_win, f"{path} after reset")
    st = _np(env.get_state().stats)  # (computed by the reset kernel)
    assert np.array_equal(st[:, SOL_LENGTH], np.maximum(length, 0)) and np.array_equal(st[:, DIST_WIN], dist_win)
    sd = env.state_dict()
    # narrow walks on from (0, 0): writing solid leaves every level alone whose cells on the way are solid already
    for _ in range(steps):
        env.step(torch.ones(n, dtype=torch.int32, device=env.device))
    own, g, solved = check("after the steps")
    same = (_np(g).reshape(grids.shape) == grids).all(axis=(1, 2))
    assert solved >= int(((length > 0) & same).sum()) >= 1
    assert np.array_equal(_np(own.length)[same], length[same])
    st = _np(env.get_state().stats)  # (kept up to date by the steps)
    assert np.array_equal(st[:, SOL_LENGTH], np.maximum(_np(own.length), 0)) and np.array_equal(st[:, DIST_WIN], _np(own.dist_win))
    # stale statistics do not matter: the even envs get a floor cell in row 0 (a second region unless it touches the room)
    env.update((torch.arange(n, device=env.device) % 2).to(torch.int32), want_obs=False)
    stale, g, _ = check("after update without refresh_stats")
    assert int((_np(stale.length) != _np(own.length)).sum()) >= 1
    assert not np.array_equal(_np(env.get_state().stats), _np(env.stats_for_grids(g)))  # (stale indeed)
    env.refresh_stats()
    st = _np(env.get_state().stats)
    assert np.array_equal(st[:, SOL_LENGTH], np.maximum(_np(stale.length), 0)) and np.array_equal(st[:, DIST_WIN], _np(stale.dist_win))
    again = env.solutions(cap=128, dist_win=True)
    assert torch.equal(again.moves, stale.moves) and torch.equal(again.length, stale.length)
    env.reset(mask=torch.as_tensor((np.arange(n) % 3 == 0).astype(np.uint8)))  # (random maps: hardly ever a level)
    masked, g, _ = check("after a masked reset")
    keep = np.arange(n) % 3 != 0
    assert np.array_equal(_np(masked.length)[keep], _np(stale.length)[keep])
    env.load_state_dict(sd)
    restored, g, _ = check("after load_state_dict")
    _check(restored, sols, length, dist_win, f"{path} after load_state_dict")
    env.check_errors()
    env.close()


# ---- caps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 16), (20, 40)], ids=["16x16", "20x40"])
def test_caps_leave_the_guard_bytes_alone(shape):
    """the raw entry point with a row of 0x77 in front of and behind the buffer: caps 1, around the longest solution, odd ones
    (rows that start at every alignment), the capacity; each again from an address that is 1 and 3 mod 4.  `length` does not
    depend on the cap."""
    grids, sols, length, dist_win = _room_file(os.path.join(SOL, f"rooms_{shape[0]}x{shape[1]}.npz"))
    env = _vec("sokoban", "narrow", shape, 4)
    L, h, n = env._L, env._h, len(grids)
    g = torch.as_tensor(grids).cuda().contiguous()
    lmax = int(length.max())
    capacity = env._L.pcgrl_solution_capacity(h)
    assert lmax >= 5 and capacity == 10000
    for cap in sorted({1, 2, 3, 7, lmax - 1, lmax, lmax + 1, 64, capacity}):
        want = torch.as_tensor(_as_array(sols, cap)).cuda()
        for shift in (0, 1, 3):
            raw = torch.full(((n + 2) * cap + shift,), 0x77, dtype=torch.int8, device="cuda")
            got_len = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            got_dw = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            ptr = raw.data_ptr() + shift + cap
            assert L.pcgrl_solutions_for_grids(h, n, g.data_ptr(), cap, ptr, got_len.data_ptr(), got_dw.data_ptr(), env._stream()) == 0
            rows = raw[shift:].view(n + 2, cap)
            what = f"{shape} cap {cap} shift {shift}"
            assert torch.equal(rows[1:-1], want), what
            assert bool((rows[0] == 0x77).all()) and bool((rows[-1] == 0x77).all()) and bool((raw[:shift] == 0x77).all()), what
            assert np.array_equal(_np(got_len), length) and np.array_equal(_np(got_dw), dist_win), what
    # no maps: a no-op; dist_win is optional; bad arguments on a live handle
    empty = env.solutions_for_grids(torch.empty((0,) + shape, dtype=torch.uint8))
    assert tuple(empty.moves.shape) == (0, capacity) and tuple(empty.length.shape) == (0,)
    p = g.data_ptr()
    assert L.pcgrl_solutions_for_grids(h, 0, None, 4, None, None, None, None) == 0
    for rc in (L.pcgrl_solutions(h, 0, p, p, None, None), L.pcgrl_solutions(h, 4, None, p, None, None),
               L.pcgrl_solutions(h, 4, p, None, None, None)):
        assert rc == 1 and b"pcgrl_solutions:" in L.pcgrl_last_error()
    for rc in (L.pcgrl_solutions_for_grids(h, -1, p, 4, p, p, None, None), L.pcgrl_solutions_for_grids(h, 1, None, 4, p, p, None, None),
               L.pcgrl_solutions_for_grids(h, 1, p, 0, p, p, None, None), L.pcgrl_solutions_for_grids(h, 1, p, 4, None, p, None, None),
               L.pcgrl_solutions_for_grids(h, 1, p, 4, p, None, None, None)):
        assert rc == 1 and b"pcgrl_solutions_for_grids:" in L.pcgrl_last_error()
    env.check_errors()
    env.close()


# ---- next to the steps --------------------------------------------------------------------------------------------------------
def test_solutions_under_a_solver_budget_with_searches_parked():
    """asynchronous stepping (set_solver_budget(16)): solutions() runs its searches to the end on the synchronous pool -- the
    answers are those of an engine without a budget --, no env's busy state changes because of the call, and the trajectory
    under step_ready stays the oracle's (the Ready driver checks every emitted transition)."""
    rep, shape, n, budget = "turtle", (16, 16), 48, 16
    env, orc = _pair(rep, shape, n, 29, False, budget, solver_power=200)
    sync = _vec("sokoban", rep, shape, 4, solver_power=200)
    maps, boxes, pos = rooms(n, shape, 5, rep)
    pol = Policy(rep, shape, boxes, 6)
    d = Ready(env, orc, False)
    d.reset(init_grids=maps, init_pos=pos)
    calls_while_busy = solved = 0
    for t in range(150):
        d.launch(pol(orc))
        if t % 5 == 0:
            busy = env.env_busy()
            out = env.solutions(cap=64, dist_win=True)
            assert torch.equal(env.env_busy(), busy), f"launch {t}: a solutions call changed an env's status"
            g = env.get_state().grids  # (a busy env's record holds the map before its step in flight: so do the planes)
            ref = sync.solutions_for_grids(g, cap=64, dist_win=True)
            for key in ("moves", "length", "dist_win"):
                assert torch.equal(getattr(out, key), getattr(ref, key)), f"launch {t}: {key}"
            solved += _consistent(sync, out, g, f"launch {t}")
            calls_while_busy += int(busy.any())
    # it searched, searches were parked while solutions() ran, and some of its answers were solutions
    assert calls_while_busy >= 3 and solved >= 1 and d.emitted > n and d.busy_launches >= 10, (calls_while_busy, solved, d.emitted)
    d.finish()
    sync.close()
    env.close()


def test_solutions_between_steps_leave_the_trajectory_the_oracles():
    """synchronous stepping on playable levels (the solver fires in the step kernel): a solutions() call after every step uses
    the same workspace pool and changes nothing the steps see"""
    rep, shape, n = "turtle", (16, 16), 32
    env, orc = _pair(rep, shape, n, 41, False, None, solver_power=400)
    maps, boxes, pos = rooms(n, shape, 8, rep)
    pol = Policy(rep, shape, boxes, 9)
    env.reset(init_grids=maps, init_pos=pos)
    orc.reset(init_grids=maps, init_pos=pos)
    fired = 0
    for t in range(40):
        a = pol(orc)
        obs, rew, done, _, info = env.step(torch.as_tensor(a, dtype=torch.int32).to(env.device))
        oobs, orew, odone, ostats = orc.step(a, auto_reset=False)
        st = _np(info["stats"])
        assert np.array_equal(st, ostats), t
        assert np.array_equal(_np(done), odone) and np.abs(_np(rew) - orew).max() <= 1e-6 and np.array_equal(_np(obs), oobs), t
        out = env.solutions(cap=64, dist_win=True)
        state = env.get_state()
        cur = _np(state.stats)
        assert np.array_equal(cur, ostats), t
        need = (cur[:, 0] == 1) & (cur[:, 1] == cur[:, 2]) & (cur[:, 1] > 0) & (cur[:, 3] == 1)
        assert np.array_equal(_np(out.length), np.where(need, cur[:, SOL_LENGTH], -1)), t
        assert np.array_equal(_np(out.dist_win), cur[:, DIST_WIN]), t
        fired += int(need.sum())
    assert fired >= 10 * n, fired
    assert np.array_equal(_np(env.get_state().grids).reshape(n, -1), orc.get_state()["grids"])
    env.check_errors()
    env.close()


def test_step_and_solutions_captured_in_one_graph():
    """"HIP-graph capturable": a step and the solutions of the stepped maps as one captured chain, replayed with fresh actions,
    the workspace pool reserved beforehand"""
    rep, shape, n = "turtle", (16, 16), 32
    env, orc = _pair(rep, shape, n, 51, False, None, solver_power=400)
    assert env.reserve_solver_pool() >= 4
    maps, boxes, pos = rooms(n, shape, 12, rep)
    pol = Policy(rep, shape, boxes, 13)
    env.reset(init_grids=maps, init_pos=pos)
    orc.reset(init_grids=maps, init_pos=pos)
    static_a = torch.zeros(n, dtype=torch.int32, device=env.device)

    def play():
        a = pol(orc)
        ostats = orc.step(a, auto_reset=False)[3]
        static_a.copy_(torch.as_tensor(a, dtype=torch.int32))
        return ostats

    for _ in range(3):  # (eager warm-up before the capture)
        play()
        env.step(static_a)
        env.solutions(cap=64, dist_win=True)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            info = env.step(static_a)[4]
            out = env.solutions(cap=64, dist_win=True)
    torch.cuda.current_stream().wait_stream(side)
    solved = 0
    for t in range(5):
        ostats = play()
        graph.replay()
        assert np.array_equal(_np(info["stats"]), ostats), t
        solved += _consistent(env, out, env.get_state().grids, f"replay {t}")
        assert np.array_equal(np.maximum(_np(out.length), 0), ostats[:, SOL_LENGTH]), t
    assert solved >= 1
    env.check_errors()
    env.close()


# ---- the other front ends -----------------------------------------------------------------------------------------------------
def test_sub_batched_solutions_equal_the_fixture():
    from control_pcgrl_amd import SubBatchedVecEnv
    grids, sols, length, dist_win = _room_file(os.path.join(SOL, "rooms_16x16.npz"))
    n = len(grids)
    four = SubBatchedVecEnv("sokoban", "narrow", (16, 16), n, sub_batches=4, seeds=9 + np.arange(n))
    four.reset(init_grids=torch.as_tensor(grids))
    out = four.solutions(cap=64, dist_win=True)
    assert tuple(out.moves.shape) == (n, 64)
    _check(out, sols, length, dist_win, "sub-batched")
    assert four.solutions(cap=5).dist_win is None
    four.close()


def test_gym_adapter_solution():
    """make_env(cfg).solution: the reference's list of {"x": dx, "y": dy} dicts; [] when no stage wins; None when the statistics
    have no "solution" key"""
    from control_pcgrl_amd import make_env
    grids, sols, length, dist_win = _room_file(os.path.join(SOL, "rooms_16x16.npz"))
    env = make_env({"task": {"problem": "sokoban", "map_shape": (16, 16)}, "representation": "narrow"})
    env.reset(seed=4)
    solved, unsolved = int(np.argmax(length > 0)), int(np.argmax(length == 0))
    no_player = grids[solved].copy()
    no_player[no_player == sr.PLAYER] = sr.EMPTY
    for g, want in ((grids[solved], [dict(sr.AS_DICTS[m]) for m in sols[solved]]), (grids[unsolved], []), (no_player, None)):
        env._vec.reset(init_grids=torch.as_tensor(g[None]))
        got = env.solution
        assert got == want and (want is None or all(type(m) is dict for m in got))
    assert length[solved] > 0 and length[unsolved] == 0
    env.close()


@pytest.mark.parametrize("problem,rep,shape", [("binary", "narrow", (16, 16)), ("zelda", "turtle", (16, 16)),
                                               ("minecraft_3D_maze", "narrow", (7, 7, 7))])
def test_problems_without_a_solver_refuse(problem, rep, shape):
    env = _vec(problem, rep, shape, 8)
    env.reset()
    assert env._L.pcgrl_solution_capacity(env._h) == 0
    with pytest.raises(NotImplementedError, match="pcgrl_solutions"):
        env.solutions()
    with pytest.raises(NotImplementedError, match="pcgrl_solutions_for_grids"):
        env.solutions_for_grids(env.get_state().grids, cap=4)
    env.check_errors()
    env.close()


def test_paths_on_sokoban_are_still_refused():
    env = _vec("sokoban", "narrow", (16, 16), 8)
    env.reset()
    assert env._L.pcgrl_path_capacity(env._h) == 0 and env._L.pcgrl_solution_capacity(env._h) == 10000
    with pytest.raises(NotImplementedError, match="pcgrl_paths"):
        env.paths()
    with pytest.raises(NotImplementedError, match="pcgrl_paths_for_grids"):
        env.paths_for_grids(env.get_state().grids, cap=4)
    assert int((env.solutions().length >= -1).sum()) == 8
    env.check_errors()
    env.close()
