"""Solution paths (include/pcgrl_amd_paths.h) on the GPU: every fixture recorded from the reference (tests/golden/paths/,
tools/gen_golden_paths.py) and fresh random maps against the numpy statement of the rules (tests/paths_numpy.py), the engine's
own maps after resets / steps / updates, short caps, the refusals, sub-batching and the gym adapter."""
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
    for _ in range(50):
        env.step(torch.randint(0, env.num_actions, (n,), generator=gen, dtype=torch.int32).cuda())
    before = check("after 50 steps")
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
