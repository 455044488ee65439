"""minecraft_3D_maze under the turtle and wide representations, the parts that need no GPU: configuration validation,
the Python shapes and spaces, and the conditions on the committed reference episodes (tests/golden/reps3d/, recorded by
tools/gen_golden_3d_reps.py)."""
import ctypes as C
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN

REPS3D = os.path.join(GOLDEN, "reps3d")
ALL = sorted(glob.glob(os.path.join(REPS3D, "*.npz")))
TURTLE = [p for p in ALL if "_turtle_" in os.path.basename(p)]
WIDE = [p for p in ALL if "_wide_" in os.path.basename(p)]
PROBLEM = "minecraft_3D_maze"


def _create(rep, shape, **kw):
    """pcgrl_create's return code for a 3-D maze configuration (validation runs before any HIP call: without a GPU a valid
    configuration ends in PCGRL_EHIP = 3)"""
    from control_pcgrl_amd import _lib
    from control_pcgrl_amd.vec_env import build_config
    patch = kw.pop("patch", None)
    cfg, _, _ = build_config(PROBLEM, rep, shape, **kw)
    if patch:
        patch(cfg)
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.pcgrl_create(C.byref(cfg), 4, 0, C.byref(h))
    msg = L.pcgrl_last_error().decode() if rc else ""
    if rc == 0:  # (a GPU is present after all)
        L.pcgrl_destroy(h)
    return rc, msg


@pytest.mark.parametrize("rep", ["turtle", "wide"])
@pytest.mark.parametrize("shape", [(7, 7, 7), (15, 15, 15), (10, 10, 10), (5, 6, 7)])
def test_create_accepts_3d_turtle_and_wide(rep, shape):
    rc, msg = _create(rep, shape)
    assert rc in (0, 3), (rc, msg)  # PCGRL_OK or PCGRL_EHIP, never EINVAL / EUNSUPPORTED


def test_wide_3d_needs_the_whole_map_as_window():
    rc, msg = _create("wide", (7, 7, 7), obs_window=(14, 14, 14))
    assert rc == 1, (rc, msg)  # PCGRL_EINVAL
    rc, msg = _create("wide", (7, 7, 7), obs_window=(7, 7, 6))
    assert rc == 1, (rc, msg)


@pytest.mark.parametrize("rep", ["narrow", "turtle", "wide"])
def test_static_tiles_and_act_window_stay_unsupported_in_3d(rep):
    def static(cfg):
        cfg.static_tiles = 1
        cfg.static_prob = 0.1

    def patch_aw(cfg):
        cfg.act_window[0] = cfg.act_window[1] = cfg.act_window[2] = 2

    for patch in (static, patch_aw):
        rc, msg = _create(rep, (7, 7, 7), patch=patch)
        assert rc == 2, (rc, msg)  # PCGRL_EUNSUPPORTED


def test_python_shapes_and_action_flattening():
    from control_pcgrl_amd import flatten_wide_action
    from control_pcgrl_amd.vec_env import _onehot_channels, build_config, obs_shape_for
    for shape in ((7, 7, 7), (5, 6, 7)):
        cfg, spec, ow = build_config(PROBLEM, "wide", shape)
        assert ow == shape
        assert obs_shape_for(cfg, spec, ow) == shape + (3,)
        assert obs_shape_for(cfg, spec, ow, "codes") == shape + (1,)
        cfg, spec, ow = build_config(PROBLEM, "turtle", shape)
        assert ow == tuple(2 * s for s in shape)
        assert obs_shape_for(cfg, spec, ow) == ow + (4,)
        assert obs_shape_for(cfg, spec, ow, "codes") == ow + (1,)
    assert _onehot_channels(PROBLEM, "wide", (7, 7, 7)) == 3 and _onehot_channels(PROBLEM, "turtle", (7, 7, 7)) == 4
    # the flat wide action: C order over (d0, d1, d2, n_tiles)
    a = np.array([[1, 2, 3, 1], [0, 0, 0, 0], [4, 5, 6, 1]])
    flat = flatten_wide_action(a, (5, 6, 7), 2)
    assert flat.dtype == np.int32 and flat.tolist() == [((1 * 6 + 2) * 7 + 3) * 2 + 1, 0, 5 * 6 * 7 * 2 - 1]
    assert np.array_equal(flat, np.ravel_multi_index(tuple(a.T), (5, 6, 7, 2)))
    assert int(flatten_wide_action([1, 2, 3, 1], (5, 6, 7), 2)) == flat[0]
    with pytest.raises(ValueError):
        flatten_wide_action([1, 2, 1], (5, 6, 7), 2)


def _stub_vec(rep, shape, obs_format="onehot", num_envs=1):
    """what the adapters read of a VecPcgrlEnv, without an engine behind it"""
    from control_pcgrl_amd.vec_env import build_config, obs_shape_for
    cfg, spec, ow = build_config(PROBLEM, rep, shape)
    n_cells = int(np.prod(shape))
    return SimpleNamespace(
        num_envs=num_envs, auto_reset=num_envs > 1, controls=[], act_window=None, action_entries=1, spec=spec, cfg=cfg,
        problem=PROBLEM, representation=rep, map_shape=tuple(shape), obs_window=ow, obs_format=obs_format,
        obs_shape=obs_shape_for(cfg, spec, ow, obs_format), stat_keys=list(spec.stat_keys),
        num_actions={"turtle": spec.n_tiles + 4, "wide": n_cells * spec.n_tiles}[rep], device="cpu")


def test_gym_adapter_spaces():
    from control_pcgrl_amd import PcgrlGymEnv
    e = PcgrlGymEnv(vec=_stub_vec("turtle", (7, 7, 7)))
    assert e.action_space.n == 6 and e.observation_space.shape == (14, 14, 14, 4)
    e = PcgrlGymEnv(vec=_stub_vec("wide", (7, 7, 7)))
    assert e.action_space.n == 343 * 2 and e.observation_space.shape == (7, 7, 7, 3)
    assert float(np.max(e.observation_space.high)) == 1.0


def test_codes_observation_bounds():
    from control_pcgrl_amd.envs import _observation_space
    sp = _observation_space(_stub_vec("wide", (7, 7, 7), "codes"), np.uint8)
    assert sp.shape == (7, 7, 7, 1) and int(sp.high.max()) == 2 and int(sp.high.min()) == 2 and int(sp.low.max()) == 0
    sp = _observation_space(_stub_vec("turtle", (7, 7, 7), "codes"), np.uint8)
    assert sp.shape == (14, 14, 14, 1) and int(sp.high.max()) == 3


# ------------------------------------------------------------------------------------------------ the committed episodes
def test_fixture_set_is_complete():
    names = {os.path.basename(p)[:-4] for p in ALL}
    for rep in ("turtle", "wide"):
        for s in (1, 2, 3):
            assert f"episode_mc3dmaze_{rep}_s{s}" in names
        assert any(n.startswith(f"shape3d_mc3dmaze_{rep}_15_") for n in names)
        assert any(n.startswith(f"shape3d_mc3dmaze_{rep}_10_") for n in names)
        assert any(n.startswith(f"control3d_mc3dmaze_{rep}_") for n in names)
    for p in ALL:
        assert os.path.getsize(p) <= 81 * 1024, p
        z = np.load(p)
        T = len(z["action"])
        assert str(z["representation"]) in ("turtle", "wide") and str(z["problem"]) == PROBLEM
        n_cells = int(np.prod(z["map_shape"]))
        for k in ("grid", "overlay"):
            assert z[k].shape == (T, n_cells), (p, k)
        for k in ("pos", "stats", "reward", "done", "changes", "iterations"):
            assert len(z[k]) == T, (p, k)
        assert z["action"].min() >= 0 and z["action"].max() < int(z["n_actions"])
        assert set(np.unique(z["overlay"])) <= {0, 1, 2} and set(np.unique(z["reset_obs"])) <= {0, 1}
    for p in ALL:
        if os.path.basename(p).startswith("episode_"):
            z = np.load(p)
            assert int(z["episode_len"]) == 7 ** 3 * 3 + 2 and len(z["action"]) > int(z["episode_len"])  # a whole episode and more
        if os.path.basename(p).startswith("shape3d_"):
            z = np.load(p)  # max_changes ends the episode
            ep = int(z["episode_len"])
            assert z["done"][ep - 1] and z["changes"][ep - 1] == int(z["max_changes"]) + 1 and z["iterations"][ep - 1] == ep


def test_wide_fixtures_exercise_the_searches():
    """at least one wide fixture has steps with n_jump > 0, and at least one a step whose path length is at least half the
    largest of stats_mc3dmaze.npz (35, so 18)"""
    longest = int(np.load(os.path.join(GOLDEN, "stats_mc3dmaze.npz"))["stats"][:, 1].max())
    assert longest == 35
    half = (longest + 1) // 2
    stats = [np.load(p)["stats"] for p in WIDE]
    assert any((s[:, 2] > 0).any() for s in stats)
    assert any((s[:, 1] >= half).any() for s in stats)


def test_scripted_wide_episodes_end_on_the_known_statistics():
    for p in WIDE:
        z = np.load(p)
        if "scripted_steps" not in z.files:
            continue
        n = int(z["scripted_steps"])
        assert np.array_equal(z["stats"][n - 1], z["scripted_stats"])
        # one cell per step in C order, no transposition: the map after the script is what the actions spell
        want = (z["action"][:n] & 1).astype(np.uint8)
        assert np.array_equal(z["action"][:n] >> 1, np.arange(n)) and np.array_equal(z["grid"][n - 1], want)


def _episodes(z):
    """[start, end) step ranges between resets"""
    starts = [int(s) for s in z["reset_step"]] + [len(z["action"])]
    return [(a, b) for a, b in zip(starts[:-1], starts[1:]) if b > a]


def test_turtle_third_coordinate_never_moves():
    """turtle_rep._dirs holds 2-tuples: the position moves along the first two axes only, the third keeps the value drawn
    at reset.  The fixtures cover an interior slab and a boundary one."""
    assert TURTLE
    third, moved = set(), False
    for p in TURTLE:
        z = np.load(p)
        d = [int(s) for s in z["map_shape"]]
        for k, (a, b) in enumerate(_episodes(z)):
            pos = z["pos"][a:b].astype(int)
            assert (pos[:, 2] == int(z["reset_pos"][k][2])).all(), (p, k)
            third.add((int(z["reset_pos"][k][2]), d[2]))
            if b - a > 500:
                assert len(np.unique(pos[:, 0])) > 1 and len(np.unique(pos[:, 1])) > 1, (p, k)
                moved = True
    assert moved
    assert any(0 < v < d2 - 1 for v, d2 in third) and any(v in (0, d2 - 1) for v, d2 in third), third


def test_turtle_fixture_semantics():
    """the recorded episodes follow the model the GPU tests step in numpy: clamped moves on axes 0 / 1, writes at the
    position, change counted iff the tile differs, statistics untouched by moves"""
    for p in TURTLE:
        z = np.load(p)
        d = [int(s) for s in z["map_shape"]]
        for k, (a, b) in enumerate(_episodes(z)):
            pos, grid = z["reset_pos"][k].astype(int).copy(), z["reset_grid"][k].copy()
            stats, changes = z["reset_stats"][k], 0
            for t in range(a, b):
                act = int(z["action"][t])
                if act < 4:
                    ax = act >> 1
                    pos[ax] = min(max(pos[ax] + (1 if act & 1 else -1), 0), d[ax] - 1)
                    assert np.array_equal(z["stats"][t], stats) and z["reward"][t] == 0
                else:
                    i = (pos[0] * d[1] + pos[1]) * d[2] + pos[2]
                    changes += int(grid[i] != act - 4)
                    grid[i] = act - 4
                stats = z["stats"][t]
                assert np.array_equal(z["pos"][t], pos) and np.array_equal(z["grid"][t], grid), (p, t)
                assert int(z["changes"][t]) == changes and int(z["iterations"][t]) == t - a + 1


def test_wide_overlay_is_the_previous_update():
    """obs["map"] of a step shows this step's edit under the path of the statistics update BEFORE it: off the path it is the
    edited map, and a step that follows one without a change shows the same path"""
    for p in WIDE:
        z = np.load(p)
        for k, (a, b) in enumerate(_episodes(z)):
            assert np.array_equal(z["reset_obs"][k], z["reset_grid"][k])
            for t in range(a, min(b, a + 400)):
                ov, g = z["overlay"][t], z["grid"][t]
                assert np.array_equal(ov[ov != 2], g[ov != 2]), (p, t)
                if t == a:  # no statistics update since the reset's: its path
                    continue
                if np.array_equal(z["grid"][t - 1], z["grid"][t - 2] if t - 2 >= a else z["reset_grid"][k]):
                    # the step before changed nothing, so no update happened in between: the same path tiles are shown
                    # wherever this step's own edit did not land
                    cell = int(z["action"][t]) >> 1
                    keep = np.arange(len(ov)) != cell
                    assert np.array_equal((ov == 2)[keep], (z["overlay"][t - 1] == 2)[keep]), (p, t)


# ------------------------------------------------------------------------------------------------ optional: the reference
@pytest.mark.reference
def test_reference_agrees_with_the_fixtures():
    """re-runs the head of one turtle and one wide fixture on the reference (build container only)"""
    import ref_env
    if not ref_env.available():
        pytest.skip("the reference tree is not present")
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), os.pardir, "tools"))
    import gen_golden_3d_reps as gg
    for name in ("episode_mc3dmaze_turtle_s1", "scripted_mc3dmaze_wide_longest_s5"):
        z = np.load(os.path.join(REPS3D, name + ".npz"))
        shape = tuple(int(s) for s in z["map_shape"])
        R = gg.Recorder(str(z["representation"]), shape, int(z["seed"]))
        R.reset()
        assert np.array_equal(R.resets["grid"][0], z["reset_grid"][0]) and np.array_equal(R.resets["pos"][0], z["reset_pos"][0])
        for t in range(400):
            R.step(int(z["action"][t]))
            assert np.array_equal(R.rec["grid"][t], z["grid"][t]) and np.array_equal(R.rec["stats"][t], z["stats"][t])
            assert np.array_equal(R.rec["overlay"][t], z["overlay"][t]) and R.rec["reward"][t] == z["reward"][t]
