"""The CPU oracle on minecraft_3D_maze under the turtle and wide representations, pinned on the reference episodes of
tests/golden/reps3d/ (recorded by tools/gen_golden_3d_reps.py).  No GPU.

Every file is replayed from its seed alone, across its mid-file reset: grid, statistics, done and both counters of every
step exactly, the position (turtle always; wide after a step, where the reference's `_pos` is the cell just edited -- its
value at a reset is stale or absent, see Recorder.pos), rewards within 1e-9 (float64 on both sides, the tolerance of
test_oracle_golden.py for controls), and the OBSERVATION of every step against the file's `overlay`, the reference's raw
obs["map"] with codes 0 AIR / 1 DIRT / 2 path: for wide the argmax over the channel axis, for turtle the window un-cropped
around the position minus one, with channel 0 set exactly outside the map.  The two control files queue their targets
from `reset_trg` and compare the control observation with rtol=1e-12, atol=0 (both sides float64), as the narrow 3-D
control file is compared in test_oracle_golden.py.

This is what lets tests/fuzz_parity.py use the oracle as the reference for these representations."""
import glob
import os

import numpy as np
import pytest

import pcgrl_oracle as po
from conftest import GOLDEN

PROBLEM = "minecraft_3D_maze"
ALL = sorted(glob.glob(os.path.join(GOLDEN, "reps3d", "*.npz")))


def test_all_sixteen_files_are_replayed():
    assert len(ALL) == 16
    reps = [os.path.basename(p).split("_mc3dmaze_")[1].split("_")[0] for p in ALL]
    assert reps.count("turtle") == 8 and reps.count("wide") == 8


def observed_map(rep, shape, obs_window, obs, pos):
    """the map of codes 0 / 1 / 2 an observation shows, after checking everything else the observation says"""
    assert obs.dtype == np.uint8 and (obs.sum(-1) == 1).all() and obs.max() == 1, "one-hot"
    codes = obs.argmax(-1)
    if rep == "wide":
        assert obs.shape == shape + (3,)
        return codes.ravel()
    assert obs.shape == tuple(obs_window) + (4,)
    # Cropped: the window starts at pos - obs_window // 2, so map cell i sits at window index i - pos + obs_window // 2
    sl = tuple(slice(w // 2 - int(p), w // 2 - int(p) + s) for s, w, p in zip(shape, obs_window, pos))
    assert all(s.start >= 0 and s.stop <= w for s, w in zip(sl, obs_window)), "the default window holds the whole map"
    inside = np.zeros(codes.shape, bool)
    inside[sl] = True
    assert np.array_equal(codes == 0, ~inside), "channel 0 exactly outside the map"
    return codes[sl].ravel() - 1


@pytest.mark.parametrize("path", ALL, ids=[os.path.basename(p)[:-4] for p in ALL])
def test_reference_episode_replay(path):
    z = np.load(path)
    rep, shape, seed = str(z["representation"]), tuple(int(s) for s in z["map_shape"]), int(z["seed"])
    assert str(z["problem"]) == PROBLEM
    kw = {}
    if "change_percentage" in z.files:
        kw["change_percentage"] = float(z["change_percentage"])
    controls = [str(c) for c in z["controls"]] if "controls" in z.files else None
    if controls:
        kw["controls"] = controls
    env = po.OracleVecEnv(PROBLEM, rep, shape, 1, seeds=[seed], **kw)
    ow = shape if rep == "wide" else tuple(int(w) for w in z["obs_window"])
    assert ow == (shape if rep == "wide" else tuple(2 * s for s in shape))
    assert env.obs_shape == ow + (3 if rep == "wide" else 4,) and env.obs_size == int(np.prod(env.obs_shape))
    T = len(z["action"])
    assert T > 100
    resets = {int(s): k for k, s in enumerate(z["reset_step"])}
    scripted = os.path.basename(path).startswith("scripted_")  # (one episode from one reset; the others reset mid-file)
    assert 0 in resets and max(resets) < T and (scripted or len(resets) >= 2), "a reset inside the file"

    def check_reset(k):
        if controls:
            env.queue_targets({c: float(v) for c, v in zip(controls, z["reset_trg"][k])})
        obs = env.reset()
        st = env.get_state()
        assert np.array_equal(st["grids"][0], z["reset_grid"][k]), f"reset {k}: grid (RNG stream)"
        if rep == "turtle":
            assert np.array_equal(st["pos"][0], z["reset_pos"][k]), f"reset {k}: position (RNG stream)"
        assert np.array_equal(st["stats"][0], z["reset_stats"][k]), f"reset {k}: stats"
        assert st["iteration"][0] == 0 and st["changes"][0] == 0
        for o in (obs[0], env.observe()[0]):  # no overlay on a reset observation, nor on observe()
            assert np.array_equal(observed_map(rep, shape, ow, o, st["pos"][0]), z["reset_obs"][k]), f"reset {k}: observation"
        if controls:
            assert int(z["reset_at"][k]) == int(z["reset_step"][k])
            assert np.allclose(env.ctrl_obs()[0], z["reset_ctrl"][k], rtol=1e-12, atol=0), f"reset {k}: ctrl obs"

    for t in range(T):
        if t in resets:
            check_reset(resets[t])
        obs, rew, done, stats = env.step([int(z["action"][t])])
        st = env.get_state()
        assert np.array_equal(st["grids"][0], z["grid"][t]), f"grid @ {t}"
        assert np.array_equal(stats[0], z["stats"][t]) and np.array_equal(st["stats"][0], z["stats"][t]), \
            f"stats @ {t}: {stats[0]} vs {z['stats'][t]}"
        assert bool(done[0]) == bool(z["done"][t]), f"done @ {t}"
        assert st["changes"][0] == z["changes"][t] and st["iteration"][0] == z["iterations"][t], f"counters @ {t}"
        assert np.array_equal(st["pos"][0], z["pos"][t]), f"pos @ {t}: {st['pos'][0]} vs {z['pos'][t]}"
        assert abs(float(rew[0]) - float(z["reward"][t])) <= 1e-9, f"reward @ {t}: {rew[0]} vs {z['reward'][t]}"
        assert np.array_equal(observed_map(rep, shape, ow, obs[0], st["pos"][0]), z["overlay"][t]), f"observation / overlay @ {t}"
        if controls:
            assert np.allclose(env.ctrl_obs()[0], z["ctrl"][t], rtol=1e-12, atol=0), f"ctrl obs @ {t}"
    assert z["done"].any() or controls or scripted, "an episode ends inside the file"
    assert (z["overlay"] == 2).any(), "the file shows path tiles"


def test_config_refusals_match_the_engine():
    """pcgrl_create refuses a 3-D wide window other than the map (tests/test_3d_reps_cpu.py); so does make_config"""
    for ow in ((14, 14, 14), (7, 7, 6)):
        with pytest.raises(ValueError):
            po.make_config(PROBLEM, "wide", (7, 7, 7), obs_window=ow)
    po.make_config(PROBLEM, "wide", (7, 7, 7), obs_window=(7, 7, 7))
    po.make_config(PROBLEM, "turtle", (7, 7, 7), obs_window=(3, 5, 4))


def _brute_obs(rep, shape, ow, grid, pos):
    """window + one-hot of a map without overlay, cell by cell"""
    if rep == "wide":
        return np.eye(3, dtype=np.uint8)[grid.reshape(shape)]
    out = np.zeros(tuple(ow) + (4,), np.uint8)
    for idx in np.ndindex(*ow):
        c = [int(p) - w // 2 + i for p, w, i in zip(pos, ow, idx)]
        inside = all(0 <= ci < s for ci, s in zip(c, shape))
        out[idx + ((int(grid.reshape(shape)[tuple(c)]) + 1) if inside else 0,)] = 1
    return out


@pytest.mark.parametrize("rep,shape,ow", [("turtle", (5, 6, 7), (3, 4, 6)), ("turtle", (1, 4, 3), (2, 9, 2)), ("turtle", (3, 1, 1), (12, 1, 1)),
                                          ("turtle", (2, 3, 4), None), ("wide", (1, 1, 3), None), ("wide", (2, 1, 2), None),
                                          ("wide", (4, 3, 5), None)])
def test_injected_resets_windows_and_masks(rep, shape, ow):
    """what the fixtures (cubic maps, default window) leave open: injected maps and positions, any turtle window, axes of
    length 1, masked resets and masked steps, against a cell-by-cell statement of the observation"""
    n = 6
    rng = np.random.default_rng(5)
    kw = {} if ow is None else {"obs_window": ow}
    env = po.OracleVecEnv(PROBLEM, rep, shape, n, seeds=np.arange(n) + 3, **kw)
    eow = shape if rep == "wide" else (ow or tuple(2 * s for s in shape))
    env.reset()
    before = env.get_state()
    grids = rng.integers(0, 2, size=(n,) + shape, dtype=np.uint8)
    pos = np.stack([rng.integers(0, s, size=n) for s in shape], axis=1).astype(np.int32)
    mask = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    obs = env.reset(mask=mask, init_grids=grids, init_pos=pos)
    st = env.get_state()
    want_stats = po.stats_for_grids(PROBLEM, grids)
    for i in range(n):
        if mask[i]:
            assert np.array_equal(st["grids"][i], grids[i].ravel()) and np.array_equal(st["stats"][i], want_stats[i])
            if rep == "turtle":
                assert np.array_equal(st["pos"][i], pos[i])
        else:
            assert np.array_equal(st["grids"][i], before["grids"][i]) and np.array_equal(st["pos"][i], before["pos"][i])
        assert np.array_equal(obs[i], _brute_obs(rep, shape, eow, st["grids"][i], st["pos"][i])), f"env {i}"
    # masked steps: the others keep everything
    n_act = 6 if rep == "turtle" else int(np.prod(shape)) * 2
    for t in range(30):
        a = rng.integers(0, n_act, size=n)
        m = (rng.random(n) < 0.6).astype(np.uint8)
        prev = env.get_state()
        env.step_masked(m, a)
        cur = env.get_state()
        for i in range(n):
            if not m[i]:
                assert np.array_equal(cur["grids"][i], prev["grids"][i]) and cur["iteration"][i] == prev["iteration"][i]
                continue
            g, p = prev["grids"][i].copy(), prev["pos"][i].copy()
            if rep == "wide":
                p = np.array(np.unravel_index(int(a[i]) // 2, shape))
                g[int(a[i]) // 2] = int(a[i]) % 2
            elif a[i] < 4:
                ax = int(a[i]) >> 1
                p[ax] = min(max(p[ax] + (1 if a[i] & 1 else -1), 0), shape[ax] - 1)
            else:
                g[np.ravel_multi_index(tuple(p), shape)] = int(a[i]) - 4
            assert np.array_equal(cur["grids"][i], g) and np.array_equal(cur["pos"][i], p), (t, i)
            assert cur["iteration"][i] == prev["iteration"][i] + 1
            assert cur["changes"][i] == prev["changes"][i] + int(not np.array_equal(g, prev["grids"][i]))
        assert np.array_equal(cur["stats"], po.stats_for_grids(PROBLEM, cur["grids"].reshape((n,) + shape)))
        obs = env.observe()
        for i in range(n):
            assert np.array_equal(obs[i], _brute_obs(rep, shape, eow, cur["grids"][i], cur["pos"][i]))
