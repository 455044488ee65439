"""Solution paths (include/pcgrl_amd_paths.h) on the GPU: every fixture recorded from the reference (tests/golden/paths/ and its
structured/ sub-folder, tools/gen_golden_paths.py) and fresh random maps against the numpy statement of the rules
(tests/paths_numpy.py), the engine's own maps after resets / steps / updates / restores on every kernel form, caps with guard
rows, the statistic against the path, graph capture, side streams, sub-batching with steps in flight, the refusals and the gym
adapter."""
import glob
import math
import os

import numpy as np
import pytest

import paths_numpy as pn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from conftest import GOLDEN  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "paths", "*.npz")))


def _vec(*a, **k):
    from control_pcgrl_amd import VecPcgrlEnv
    return VecPcgrlEnv(*a, **k)


def _env_for(problem, shape, n=4):
    """an engine for `shape`.  zelda's static nearest-enemy target is the range (5, ceil(w / 2 + 1) * h), which is empty on a
    1 x 1 or 1 x 5 map: the reference's loss fails on it and the engine refuses the config.  The path is a function of the map
    alone, so those two shapes get a target range of their own."""
    kw = {}
    if problem == "zelda" and math.ceil(shape[1] / 2 + 1) * shape[0] <= 5:
        kw["static_trgs"] = {"nearest-enemy": (0, 1)}
    return _vec(problem, "narrow", shape, n, **kw)


def _lanes_per_map(shape):
    h, w = shape
    lpe = 8 if h <= 8 else 16 if h <= 16 else 32 if h <= 32 else 64
    return max(lpe, 32) if w > 32 else lpe


def _check(out, paths, shape, cap, what):
    """a paths() result against lists of cells"""
    coords, length, overlay = pn.as_arrays(paths, cap, shape)
    got_len = out.length.cpu().numpy()
    assert out.coords.shape == coords.shape and out.coords.dtype == torch.int16 and out.length.dtype == torch.int32
    bad = np.nonzero(got_len != length)[0]
    assert bad.size == 0, f"{what}: length differs in {bad.size} maps, first {bad[:5]}: {got_len[bad[:5]]} != {length[bad[:5]]}"
    bad = np.nonzero((out.coords.cpu().numpy() != coords).any(axis=(1, 2)))[0]
    assert bad.size == 0, f"{what}: cells differ in {bad.size} maps, first {bad[:5]}"
    if out.overlay is not None:
        assert out.overlay.dtype == torch.uint8 and tuple(out.overlay.shape) == overlay.shape
        bad = np.nonzero((out.overlay.cpu().numpy() != overlay).any(axis=(1, 2)))[0]
        assert bad.size == 0, f"{what}: overlay differs in {bad.size} maps, first {bad[:5]}"


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_fixtures_through_paths_for_grids(path):
    z = np.load(path)
    problem, hw = os.path.basename(path)[:-4].split("_")
    shape = tuple(int(s) for s in hw.split("x"))
    grids, cells, off = z["grids"], z["cells"], z["offsets"]
    paths = [[tuple(c) for c in cells[off[i]:off[i + 1]].tolist()] for i in range(len(grids))]
    env = _env_for(problem, shape)
    cap = 2 * shape[0] * shape[1] if problem == "zelda" else shape[0] * shape[1]
    assert env._L.pcgrl_path_capacity(env._h) == cap
    # the whole file in one call; then counts that leave the last wavefront partly filled
    epw = 64 // _lanes_per_map(shape)
    for n in (len(grids), epw + 3, 5 if epw == 8 else 3):
        out = env.paths_for_grids(torch.as_tensor(grids[:n]), overlay=True)
        _check(out, paths[:n], shape, cap, f"{os.path.basename(path)} n={n}")
    if problem == "binary":  # L is the engine's path-length statistic
        st = env.stats_for_grids(torch.as_tensor(grids)).cpu().numpy()
        assert np.array_equal(st[:, env.stat_keys.index("path-length")], z["L"])
    env.check_errors()
    env.close()


@pytest.mark.parametrize("problem,shape,n", [("binary", (16, 16), 1000), ("zelda", (16, 16), 1000),
                                             ("binary", (40, 48), 64), ("zelda", (40, 48), 64)])
def test_random_maps_against_the_numpy_rules(problem, shape, n):
    grids = pn.random_maps(problem, n, shape, np.random.default_rng(20261017 + n + (problem == "zelda")))
    paths = [pn.path_of(problem, g) for g in grids]
    env = _vec(problem, "narrow", shape, 4)
    g = torch.as_tensor(grids, device=env.device)
    out = env.paths_for_grids(g, overlay=True)
    _check(out, paths, shape, out.coords.shape[1], f"{problem} {shape}")
    assert sum(len(p) > 0 for p in paths) > n // 4
    if problem == "binary":
        pl = env.stats_for_grids(g)[:, env.stat_keys.index("path-length")]
        assert torch.equal(torch.where(pl > 0, pl + 1, torch.zeros_like(pl)), out.length)
        assert torch.equal(out.length == 0, pl == 0)
    env.check_errors()
    env.close()


def _same(a, b, what):
    assert torch.equal(a.length, b.length), what
    assert torch.equal(a.coords, b.coords), what
    assert torch.equal(a.overlay, b.overlay), what


@pytest.mark.parametrize("problem,rep", [("binary", "narrow"), ("zelda", "turtle")])
def test_paths_of_the_engines_own_maps(problem, rep):
    n = 256
    env = _vec(problem, rep, (16, 16), n, seeds=5 + np.arange(n), auto_reset=True)
    gen = torch.Generator().manual_seed(3)
    if problem == "zelda":  # (the engine's random zelda maps hardly ever hold exactly one player, key and door)
        env.reset(init_grids=pn.random_maps(problem, n, (16, 16), np.random.default_rng(8)))
    else:
        env.reset()

    def check(what, sample=8):
        grids = env.get_state().grids
        own = env.paths(overlay=True)
        _same(own, env.paths_for_grids(grids, overlay=True), what)
        idx = list(range(0, n, n // sample))
        sub = [pn.path_of(problem, g) for g in grids.cpu().numpy()[idx]]
        coords, length, overlay = pn.as_arrays(sub, own.coords.shape[1], (16, 16))
        assert np.array_equal(own.length.cpu().numpy()[idx], length), what
        assert np.array_equal(own.coords.cpu().numpy()[idx], coords), what
        assert np.array_equal(own.overlay.cpu().numpy()[idx], overlay), what
        return own

    assert int((check("after reset").length > 0).sum()) > n // 4
    # zelda's tile actions place only empty, solid and enemies (draw_actions): with uniform tiles 11 of the 256 maps still had
    # a path after the 50 steps, with these the CPU oracle alone (same seeds, maps and actions) keeps 151
    for _ in range(50):
        env.step(draw_actions(problem, rep, (16, 16), n, gen).cuda())
    before = check("after 50 steps", sample=n)  # (the numpy rules on every env)
    assert int((before.length > 0).sum()) >= n // 4
    if problem == "binary":  # (length - 1 is the statistic the steps kept up to date)
        pl = env.get_state().stats[:, env.stat_keys.index("path-length")]
        assert torch.equal(torch.where(pl > 0, pl + 1, torch.zeros_like(pl)), before.length)
    # stale statistics do not matter: maps edited by update(), nothing refreshed
    for _ in range(5):
        env.update(torch.randint(0, env.num_actions, (n,), generator=gen, dtype=torch.int32).cuda(), want_obs=False)
    stale = check("after update without refresh_stats")
    if problem == "binary":
        assert not torch.equal(stale.coords, before.coords)
    env.refresh_stats()
    _same(env.paths(overlay=True), stale, "after refresh_stats")
    env.check_errors()
    env.close()


@pytest.mark.parametrize("problem", ["binary", "zelda"])
def test_short_cap_no_overlay_and_no_maps(problem):
    z = np.load(os.path.join(GOLDEN, "paths", f"{problem}_16x16.npz"))
    grids = torch.as_tensor(z["grids"])
    env = _vec(problem, "narrow", (16, 16), 4)
    full = env.paths_for_grids(grids, overlay=True)
    longest = int(full.length.max())
    assert longest > 9
    for cap in (1, 7, 16, longest - 1):  # (7: sets of 16 cells cut in the middle; 16: exactly one set)
        cut = env.paths_for_grids(grids, cap=cap, overlay=True)
        assert tuple(cut.coords.shape) == (len(grids), cap, 2)
        assert torch.equal(cut.length, full.length)
        assert torch.equal(cut.coords, full.coords[:, :cap])
        assert torch.equal(cut.overlay, full.overlay)  # (complete, also past cap)
    none = env.paths_for_grids(grids, cap=7)
    assert none.overlay is None and torch.equal(none.coords, full.coords[:, :7])
    empty = env.paths_for_grids(torch.empty((0, 16, 16), dtype=torch.uint8))
    assert tuple(empty.coords.shape) == (0, full.coords.shape[1], 2) and tuple(empty.length.shape) == (0,)
    # a buffer of int16 pairs that is not 4-byte aligned
    L, h, n, cap = env._L, env._h, len(grids), 9
    g = grids.cuda().contiguous()
    raw = torch.full((n * cap * 2 + 1,), 7, dtype=torch.int16, device="cuda")
    length = torch.empty(n, dtype=torch.int32, device="cuda")
    assert L.pcgrl_paths_for_grids(h, n, g.data_ptr(), cap, raw.data_ptr() + 2, length.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert raw[0] == 7 and torch.equal(raw[1:].view(n, cap, 2), full.coords[:, :cap])
    # bad arguments on a live handle
    p = raw.data_ptr()
    for rc in (L.pcgrl_paths(h, 0, p, p, None, None), L.pcgrl_paths(h, 4, None, p, None, None),
               L.pcgrl_paths(h, 4, p, None, None, None)):
        assert rc == 1 and b"pcgrl_paths:" in L.pcgrl_last_error()
    for rc in (L.pcgrl_paths_for_grids(h, -1, p, 4, p, p, None, None), L.pcgrl_paths_for_grids(h, 1, None, 4, p, p, None, None),
               L.pcgrl_paths_for_grids(h, 1, p, 0, p, p, None, None), L.pcgrl_paths_for_grids(h, 1, p, 4, None, p, None, None)):
        assert rc == 1 and b"pcgrl_paths_for_grids:" in L.pcgrl_last_error()
    env.check_errors()
    env.close()


@pytest.mark.parametrize("problem,rep,shape", [("sokoban", "narrow", (16, 16)), ("minecraft_3D_maze", "narrow", (7, 7, 7))])
def test_problems_without_a_path_refuse(problem, rep, shape):
    env = _vec(problem, rep, shape, 8)
    env.reset()
    assert env._L.pcgrl_path_capacity(env._h) == 0
    with pytest.raises(NotImplementedError, match="pcgrl_paths"):
        env.paths()
    with pytest.raises(NotImplementedError, match="pcgrl_paths_for_grids"):
        env.paths_for_grids(env.get_state().grids, cap=4)
    env.check_errors()
    env.close()


@pytest.mark.parametrize("problem,rep", [("binary", "narrow"), ("zelda", "turtle")])
def test_sub_batched_paths_equal_the_single_engine(problem, rep):
    from control_pcgrl_amd import SubBatchedVecEnv
    n = 64
    seeds = 9 + np.arange(n)
    one = _vec(problem, rep, (16, 16), n, seeds=seeds)
    four = SubBatchedVecEnv(problem, rep, (16, 16), n, sub_batches=4, seeds=seeds)
    # (the engine's random zelda maps hardly ever hold exactly one player, key and door)
    kw = {"init_grids": torch.as_tensor(pn.random_maps(problem, n, (16, 16), np.random.default_rng(2)))} if problem == "zelda" else {}
    one.reset(**kw)
    four.reset(**kw)
    assert torch.equal(one.get_state().grids, four.get_state().grids)
    a, b = one.paths(overlay=True), four.paths(overlay=True)
    _same(a, b, "sub-batched")
    assert int(a.length.max()) > 0
    assert four.paths(cap=5).overlay is None
    one.close()
    four.close()


@pytest.mark.parametrize("problem,rep", [("binary", "narrow"), ("zelda", "turtle")])
def test_gym_adapter_path_coords(problem, rep):
    from control_pcgrl_amd import make_env
    env = make_env({"task": {"problem": problem, "map_shape": (16, 16)}, "representation": rep})
    env.reset(seed=4)
    env.step(1)
    got = env.path_coords
    want = pn.path_of(problem, env.get_map())
    assert got.dtype == np.int32 and got.shape == (len(want), 2)
    assert [tuple(c) for c in got.tolist()] == want
    row0 = env._vec.paths()
    assert np.array_equal(row0.coords[0, :int(row0.length[0])].cpu().numpy(), got)
    env.close()


# ---- every kernel form, from the engine's own planes and from caller bytes ------------------------------------------------------
STRUCTURED = sorted(glob.glob(os.path.join(GOLDEN, "paths", "structured", "*.npz")))
# one shape per (lanes per map, mask bits) form: 8/32, 16/32, 32/32, 64/32, 32/64, 64/64, and the representation stepped on it
# (wide needs a square map, as the reference's transposed write does; on 8 x 8 narrow and wide overwrite zelda's player, key
# or door within the 40 steps of test_own_maps_on_every_form, the turtle mostly walks)
FORMS = [((8, 8), "turtle"), ((16, 16), "wide"), ((20, 24), "narrow"), ((40, 16), "narrow"), ((12, 40), "narrow"),
         ((40, 48), "narrow")]
ZELDA_KEPT = (0, 1, 5, 6, 7)  # empty, solid and the enemies: tile actions that leave the one player, key and door alone


def _shape_id(shape):
    return f"{shape[0]}x{shape[1]}"


def _structured(problem, shape):
    """-> (grids, the recorded paths as lists of cells) of tests/golden/paths/structured/<problem>_<H>x<W>.npz"""
    z = np.load(os.path.join(GOLDEN, "paths", "structured", f"{problem}_{_shape_id(shape)}.npz"))
    cells, off = z["cells"], z["offsets"]
    return z["grids"], [[tuple(c) for c in cells[off[i]:off[i + 1]].tolist()] for i in range(len(z["grids"]))]


def draw_actions(problem, rep, shape, n, gen):
    """int32 [n] uniform actions (CPU); zelda's tile actions only place ZELDA_KEPT, its turtle moves are unrestricted: uniform
    tiles soon add a second player, key or door and the path is gone"""
    nt = 2 if problem == "binary" else 8
    n_act = {"narrow": nt, "turtle": nt + 4, "wide": shape[0] * shape[1] * nt}[rep]
    if problem == "binary":
        return torch.randint(0, n_act, (n,), generator=gen, dtype=torch.int32)
    kept = torch.tensor(ZELDA_KEPT, dtype=torch.int32)
    if rep == "turtle":
        a = torch.randint(0, 4 + len(kept), (n,), generator=gen, dtype=torch.int32)
        return torch.where(a < 4, a, 4 + kept[(a - 4).clamp(min=0).long()])
    tile = kept[torch.randint(0, len(kept), (n,), generator=gen).long()]
    if rep == "narrow":
        return tile
    return torch.randint(0, shape[0] * shape[1], (n,), generator=gen, dtype=torch.int32) * nt + tile


def _numpy_check(out, problem, grids, shape, what):
    """a paths() result of `grids` (a tensor) against the numpy rules, every map; -> number of non-empty paths"""
    paths = [pn.path_of(problem, g) for g in grids.cpu().numpy().reshape((-1,) + tuple(shape))]
    _check(out, paths, shape, out.coords.shape[1], what)
    return sum(len(p) > 0 for p in paths)


@pytest.mark.parametrize("path", STRUCTURED, ids=[os.path.basename(f)[:-4] for f in STRUCTURED])
def test_structured_fixtures_from_caller_bytes_and_from_the_engines_planes(path):
    """the hand-built families (spirals, serpentines with both zelda halves, tied components and routes, one- and two-cell
    maps, the key and the door at every distance 1..7) through paths_for_grids and, after reset(init_grids), through paths"""
    problem, hw = os.path.basename(path)[:-4].split("_")
    shape = tuple(int(s) for s in hw.split("x"))
    grids, paths = _structured(problem, shape)
    env = _vec(problem, "narrow", shape, len(grids))
    cap = env._L.pcgrl_path_capacity(env._h)
    assert cap == (2 if problem == "zelda" else 1) * shape[0] * shape[1]
    _check(env.paths_for_grids(torch.as_tensor(grids), overlay=True), paths, shape, cap, f"{problem} {shape} caller bytes")
    env.reset(init_grids=torch.as_tensor(grids))
    assert np.array_equal(env.get_state().grids.cpu().numpy(), grids)
    _check(env.paths(overlay=True), paths, shape, cap, f"{problem} {shape} own planes")
    env.check_errors()
    env.close()


# seeds of test_own_maps_on_every_form: engine seeds OWN_SEED + i, zelda's injected maps default_rng(OWN_MAPS), actions
# torch.Generator().manual_seed(OWN_ACTIONS).  With these the CPU oracle alone (OracleVecEnv, same seeds, maps and actions) has,
# after the 40 steps, a non-empty path in at least 99 // 4 envs on every form:
#   binary 99 / 99 on all six; zelda 8x8 47, 16x16 44, 20x24 38, 40x16 54, 12x40 41, 40x48 47 of 99
OWN_N, OWN_STEPS, OWN_SEED, OWN_MAPS, OWN_ACTIONS = 99, 40, 11, 21, 31


@pytest.mark.parametrize("shape,rep", FORMS, ids=[_shape_id(s) + "-" + r for s, r in FORMS])
@pytest.mark.parametrize("problem", ["binary", "zelda"])
def test_own_maps_on_every_form(problem, shape, rep):
    """paths() reads the engine's tile planes (load_planes), paths_for_grids the bytes get_state() hands out: the two must
    agree, on all three outputs, after a reset, after steps, after update() without refresh_stats(), after a masked reset and
    after load_state_dict.  99 envs leave the last wavefront partly filled wherever a wavefront holds several maps."""
    n = OWN_N
    env = _vec(problem, rep, shape, n, seeds=OWN_SEED + np.arange(n), auto_reset=True)
    gen = torch.Generator().manual_seed(OWN_ACTIONS)
    if problem == "zelda":
        env.reset(init_grids=pn.random_maps(problem, n, shape, np.random.default_rng(OWN_MAPS)))
    else:
        env.reset()

    def check(what):
        own = env.paths(overlay=True)
        _same(own, env.paths_for_grids(env.get_state().grids, overlay=True), f"{problem} {rep} {shape} {what}")
        return own

    first = check("after reset")
    sd = env.state_dict()
    for _ in range(OWN_STEPS):
        env.step(draw_actions(problem, rep, shape, n, gen).to(env.device))
    stepped = check("after the steps")
    nonempty = _numpy_check(stepped, problem, env.get_state().grids, shape, f"{problem} {rep} {shape} after the steps")
    assert nonempty >= n // 4, nonempty
    for _ in range(5):
        env.update(draw_actions(problem, rep, shape, n, gen).to(env.device), want_obs=False)
    check("after update without refresh_stats")
    env.reset(mask=torch.as_tensor((np.arange(n) % 3 == 0).astype(np.uint8)))
    check("after a masked reset")
    env.load_state_dict(sd)
    _same(check("after load_state_dict"), first, "the snapshot's paths")
    env.check_errors()
    env.close()


@pytest.mark.parametrize("shape", [s for s, _ in FORMS], ids=[_shape_id(s) for s, _ in FORMS])
@pytest.mark.parametrize("problem", ["binary", "zelda"])
def test_caps_on_every_form_leave_the_guard_rows_alone(problem, shape):
    """the raw entry point with a row of 0x7777 in front of and behind the buffer, at the caps where the stores of LPE cells
    are cut differently: inside the first set, at its end, one past it, around the longest path, the capacity, beyond it.
    The forms with 64-bit masks run a second time from an address that is 2 mod 4 (two shorts per cell, not one dword)."""
    grids, paths = _structured(problem, shape)
    env = _vec(problem, "narrow", shape, 4)
    L, h, n = env._L, env._h, len(grids)
    g = torch.as_tensor(grids).cuda().contiguous()
    full = env.paths_for_grids(g, overlay=True)
    capacity = full.coords.shape[1]
    _check(full, paths, shape, capacity, f"{problem} {shape}")
    lpe, lmax = _lanes_per_map(shape), int(full.length.max())
    assert lmax == max(len(p) for p in paths) and 2 * lmax >= shape[0] * shape[1]
    caps = sorted({1, lpe - 1, lpe, lpe + 1, lmax - 1, lmax, lmax + 1, capacity, capacity + lpe + 3})
    for shift in ((0, 1) if shape[1] > 32 else (0,)):
        for cap in caps:
            raw = torch.full(((n + 2) * cap * 2 + shift,), 0x7777, dtype=torch.int16, device="cuda")
            length = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            overlay = torch.full((n,) + shape, 9, dtype=torch.uint8, device="cuda")
            ptr = raw.data_ptr() + 2 * (shift + cap * 2)
            assert ptr % 4 == 2 * shift
            assert L.pcgrl_paths_for_grids(h, n, g.data_ptr(), cap, ptr, length.data_ptr(), overlay.data_ptr(), env._stream()) == 0
            rows = raw[shift:].view(n + 2, cap, 2)
            want = torch.full((n, cap, 2), -1, dtype=torch.int16, device="cuda")
            want[:, :min(cap, capacity)] = full.coords[:, :cap]
            what = f"{problem} {shape} cap {cap} shift {shift}"
            assert torch.equal(rows[1:-1], want), what
            assert bool((rows[0] == 0x7777).all()) and bool((rows[-1] == 0x7777).all()) and bool((raw[:shift] == 0x7777).all()), what
            assert torch.equal(length, full.length) and torch.equal(overlay, full.overlay), what
    env.check_errors()
    env.close()


STAT_FORMS = [(8, 8), (20, 24), (40, 16), (12, 40)]  # (test_random_maps_against_the_numpy_rules has 16 x 16 and 40 x 48)


@pytest.mark.parametrize("shape", STAT_FORMS, ids=[_shape_id(s) for s in STAT_FORMS])
@pytest.mark.parametrize("problem", ["binary", "zelda"])
def test_statistic_and_path_agree(problem, shape):
    """the path-length statistic of stats_for_grids measures the path that paths_for_grids returns.  binary: length ==
    path-length + 1, or 0 where path-length is 0.  zelda, on the maps with exactly one player, key and door: path-length ==
    dA + dB, the BFS distances player -> key (not through the door) and key -> door, each -1 where unreached
    (zelda_ctrl_prob.py:140-151)."""
    n = 64
    grids = pn.random_maps(problem, n, shape, np.random.default_rng(77 + shape[0] * 64 + shape[1] + (problem == "zelda")))
    env = _vec(problem, "narrow", shape, 4)
    g = torch.as_tensor(grids, device=env.device)
    out = env.paths_for_grids(g, overlay=True)
    assert _numpy_check(out, problem, g, shape, f"{problem} {shape}") >= n // 4
    pl = env.stats_for_grids(g)[:, env.stat_keys.index("path-length")]
    if problem == "binary":
        assert torch.equal(torch.where(pl > 0, pl + 1, torch.zeros_like(pl)), out.length)
    else:
        pl, one_each = pl.cpu().numpy(), 0
        for i, m in enumerate(grids):
            spots = [np.argwhere(m == t) for t in (pn.PLAYER, pn.KEY, pn.DOOR)]
            if all(len(s) == 1 for s in spots):
                p, k, d = (tuple(int(v) for v in s[0]) for s in spots)
                da = pn.bfs((m != pn.SOLID) & (m != pn.DOOR), p)[k]
                db = pn.bfs(m != pn.SOLID, k)[d]
                assert pl[i] == da + db, (i, pl[i], da, db)
                one_each += 1
        assert one_each >= n // 2, one_each
    env.check_errors()
    env.close()


# ---- the header's claims about streams and capture ----------------------------------------------------------------------------
def _reset_for(env, problem, shape, n, seed):
    if problem == "zelda":  # (the engine's random zelda maps hardly ever hold exactly one player, key and door)
        return env.reset(init_grids=pn.random_maps(problem, n, shape, np.random.default_rng(seed)))
    return env.reset()


@pytest.mark.parametrize("problem,shape", [("binary", (16, 16)), ("zelda", (12, 40))])
def test_step_and_paths_captured_in_one_graph(problem, shape):
    """"HIP-graph capturable": a step and the paths of the stepped maps as one captured chain, replayed with fresh actions
    (the warm-up and capture of test_step_graph_replay_vs_oracle)"""
    n = 64
    env = _vec(problem, "narrow", shape, n, seeds=70 + np.arange(n), auto_reset=True)
    _reset_for(env, problem, shape, n, 71)
    gen = torch.Generator().manual_seed(72)
    static_a = torch.zeros(n, dtype=torch.int32, device=env.device)
    for _ in range(3):  # (eager warm-up before the capture)
        env.step(draw_actions(problem, "narrow", shape, n, gen).to(env.device))
        env.paths(overlay=True)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            env.step(static_a)
            out = env.paths(overlay=True)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for t in range(5):
        static_a.copy_(draw_actions(problem, "narrow", shape, n, gen))
        graph.replay()
        grids = env.get_state().grids
        nonempty = _numpy_check(out, problem, grids, shape, f"{problem} replay {t}")
        assert nonempty >= n // 4, nonempty
        seen.append(grids.clone())
    assert not torch.equal(seen[0], seen[-1])  # (the replays did step)
    env.check_errors()
    env.close()


@pytest.mark.parametrize("problem,shape", [("binary", (16, 16)), ("zelda", (12, 40))])
def test_paths_on_a_side_stream(problem, shape):
    """"one launch on the current stream": issued under another stream that waits for the step on the default stream, the
    call sees the stepped maps and gives what the default stream gives"""
    n = 64
    env = _vec(problem, "narrow", shape, n, seeds=80 + np.arange(n), auto_reset=True)
    _reset_for(env, problem, shape, n, 81)
    gen = torch.Generator().manual_seed(82)
    side = torch.cuda.Stream()
    for t in range(4):
        for _ in range(5):
            env.step(draw_actions(problem, "narrow", shape, n, gen).to(env.device))
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            there = env.paths(overlay=True)
        torch.cuda.current_stream().wait_stream(side)
        here = env.paths(overlay=True)
        _same(there, here, f"{problem} round {t}")
    assert _numpy_check(there, problem, env.get_state().grids, shape, problem) >= n // 4
    env.check_errors()
    env.close()


@pytest.mark.parametrize("problem,rep,shape", [("binary", "narrow", (16, 16)), ("zelda", "turtle", (16, 16)),
                                               ("binary", "wide", (48, 48)), ("binary", "narrow", (40, 48))])
def test_paths_between_steps_leave_the_trajectory_alone(problem, rep, shape):
    """a paths() after every step and a paths_for_grids() of 1000 foreign maps every tenth: statistics, rewards, dones and
    observations of every step and the final state are the CPU oracle's, which computes no paths.  (The wide representation
    exists on square maps only -- pcgrl_create refuses 40 x 48 as the reference's transposed write fails on it -- so wide runs
    at 48 x 48, the same 64 lanes / 64-bit masks form, and 40 x 48 runs narrow.)"""
    import pcgrl_oracle as po
    n, steps = 64, 60
    seeds = 90 + np.arange(n)
    env = _vec(problem, rep, shape, n, seeds=seeds, auto_reset=True)
    orc = po.OracleVecEnv(problem, rep, shape, n, seeds=seeds, threads=8)
    obs, _ = env.reset()
    assert np.array_equal(obs.cpu().numpy(), orc.reset())
    foreign = torch.as_tensor(pn.random_maps(problem, 1000, shape, np.random.default_rng(91)), device=env.device)
    foreign_paths = env.paths_for_grids(foreign, overlay=True)
    gen = torch.Generator().manual_seed(92)
    for t in range(steps):
        a = torch.randint(0, env.num_actions, (n,), generator=gen, dtype=torch.int32)
        obs, rew, done, _, info = env.step(a.to(env.device))
        own = env.paths(overlay=True)
        if t % 10 == 9:
            _same(env.paths_for_grids(foreign, overlay=True), foreign_paths, f"foreign maps @ {t}")
        oobs, orew, odone, ostats = orc.step(a.numpy(), auto_reset=True)
        assert np.array_equal(info["stats"].cpu().numpy(), ostats), f"stats @ {t}"
        assert np.max(np.abs(rew.cpu().numpy().astype(np.float64) - orew)) <= 1e-6, f"reward @ {t}"
        assert np.array_equal(done.cpu().numpy(), odone), f"done @ {t}"
        assert np.array_equal(obs.cpu().numpy(), oobs), f"obs @ {t}"
    st, ost = env.get_state(), orc.get_state()
    assert np.array_equal(st.grids.cpu().numpy().reshape(n, -1), ost["grids"])
    if rep != "wide":
        assert np.array_equal(st.pos.cpu().numpy()[:, :2], ost["pos"][:, :2])
    for key in ("iteration", "changes", "n_step", "ep_len", "stats", "last_loss"):
        assert np.array_equal(getattr(st, key).cpu().numpy(), ost[key]), key
    assert np.allclose(st.ep_return.cpu().numpy(), ost["ep_return"], atol=1e-6)
    _same(own, env.paths_for_grids(st.grids, overlay=True), "the last step's paths")
    env.check_errors()
    env.close()


@pytest.mark.parametrize("problem,rep", [("binary", "narrow"), ("zelda", "turtle")])
def test_sub_batched_paths_wait_for_steps_in_flight(problem, rep):
    """SubBatchedVecEnv.paths right after step_async on every sub-batch, no wait(): each sub-batch's paths are ordered after
    its own step, so the result is the single engine's after step()"""
    from control_pcgrl_amd import SubBatchedVecEnv
    n, shape = 64, (16, 16)
    seeds = 60 + np.arange(n)
    one = _vec(problem, rep, shape, n, seeds=seeds)
    four = SubBatchedVecEnv(problem, rep, shape, n, sub_batches=4, seeds=seeds)
    kw = {"init_grids": torch.as_tensor(pn.random_maps(problem, n, shape, np.random.default_rng(61)))} if problem == "zelda" else {}
    one.reset(**kw)
    four.reset(**kw)
    gen = torch.Generator().manual_seed(62)
    for t in range(6):
        a = draw_actions(problem, rep, shape, n, gen).to(one.device)
        one.step(a)
        for i in range(4):
            four.step_async(i, a[i * (n // 4):(i + 1) * (n // 4)])
        got = four.paths(overlay=True)
        _same(one.paths(overlay=True), got, f"{problem} round {t}")
    assert torch.equal(one.get_state().grids, four.get_state().grids)
    assert int((got.length > 0).sum()) >= n // 4
    one.check_errors()
    four.check_errors()
    one.close()
    four.close()
