"""Super Mario Bros behind the VectorEnv call shape (smb_rllib.SmbVectorEnv, include/pcgrl_amd_smb_vector.h), the part that
needs no GPU: the layout of a call's block, every refusal with its reason, the dispatch of make_vector_env, the new C entry
points on null handles, and the numpy statement of the float32 image (tests/smb_vector_rules.py) that the GPU tests compare the
hand-out kernel with."""
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smb_env_rules as E  # noqa: E402
import smb_levels as sl  # noqa: E402
import smb_vector_rules as V  # noqa: E402

from control_pcgrl_amd import _lib, rllib_env, smb_env, smb_rllib  # noqa: E402

WINDOWS = [(8, 10), (9, 13), (5, 9), (32, 232)]


def cfg_of(rep="narrow", shape=(16, 116), **kw):
    task = NS(name="smb", problem="smb", map_shape=shape, obs_window=kw.pop("obs_window", None), weights=None, controls=None,
              solver_budget=kw.pop("solver_budget", 0))
    base = dict(representation=rep, task=task, controls=None, change_percentage=None, max_board_scans=3, n_aux_tiles=0,
                static_prob=None, n_static_walls=None, act_window=None, show_agents=False,
                multiagent=NS(n_agents=0, policies="centralized"))
    base.update(kw)
    return NS(**base)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n_ctrl", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 3, 20, 70])
def test_block_layout(window, n_ctrl, n):
    """[obs | reward64 | stats | done]: every section on 16 bytes, none overlapping the next, the block ending after `done`"""
    for per_env in (window[0] * window[1] * (2 * n_ctrl + 8) * 4, window[0] * window[1] * 8):
        lay = smb_rllib.block_layout(n, per_env)
        assert lay.obs == 0 and all(x % 16 == 0 for x in (lay.rew, lay.stats, lay.done, lay.total))
        assert n * per_env <= lay.rew < n * per_env + 16
        assert lay.rew + n * 8 <= lay.stats < lay.rew + n * 8 + 16
        assert lay.stats + n * 9 * 4 <= lay.done < lay.stats + n * 9 * 4 + 16
        assert lay.done + n <= lay.total < lay.done + n + 16


def test_the_alignment_cases_are_all_among_the_shapes():
    """the shapes of the GPU tests reach every store case of the kernel; the third one puts odd envs on 8 bytes only"""
    seen = {V.alignment_case(k, w) for k in (0, 1, 2) for w in WINDOWS}
    assert seen == {"Keven", "Kodd-cells-even", "Kodd-cells-odd"}
    for k in (0, 1, 2):
        for w in WINDOWS:
            floats = w[0] * w[1] * (2 * k + 8)
            assert floats % 2 == 0  # an env's run always starts on 8 bytes
            assert (floats % 4 == 0) == (V.alignment_case(k, w) != "Kodd-cells-odd")


def test_every_refusal_names_its_reason():
    def refused(match, *a, **kw):
        with pytest.raises(NotImplementedError, match=match):
            smb_rllib.SmbVectorEnv(*a, **kw)

    for budget in (64, np.int64(64), np.float32(8), "64"):  # however the cfg spells it, and before anything is built
        refused("solver budget.*synchronous", cfg_of(solver_budget=budget), 2)
    refused("solver budget.*synchronous", vec=NS(solver_budget=64, auto_reset=False))
    refused("auto_reset=True.*reset_at", vec=NS(auto_reset=True))
    # what make_vec_env refuses for smb, through it
    refused("wide", cfg_of("wide"), 2)
    refused("obs_window.*255", cfg_of(obs_window=(32, 256)), 2)
    refused("controls", cfg_of(controls=["enemies"]), 2)
    refused("static tiles", cfg_of(static_prob=0.1), 2)
    refused("act_window", cfg_of(act_window=(3, 3)), 2)
    refused("multiagent", cfg_of("turtle", multiagent=NS(n_agents=2, policies="centralized")), 2)
    refused("codes", cfg_of(obs_format="codes"), 2)
    with pytest.raises(ValueError, match="PcgrlVectorEnv"):
        smb_rllib.SmbVectorEnv(NS(task=NS(problem="binary")), 2)
    # sub-batches, which make_vec_env refuses for smb, have no argument in either entry: a TypeError names it
    for fn in (smb_rllib.SmbVectorEnv, smb_rllib.make_vector_env):
        with pytest.raises(TypeError, match="sub_batches"):
            fn(cfg_of(), 4, sub_batches=2)


def test_a_budget_that_reaches_the_env_is_refused_too(monkeypatch):
    """whatever make_vec_env builds from the cfg: an env with a budget set is closed and refused, never wrapped"""
    closed = []
    fake = NS(solver_budget=7, auto_reset=False, close=lambda: closed.append(1))
    monkeypatch.setattr(smb_rllib, "make_vec_env", lambda *a, **kw: fake)
    with pytest.raises(NotImplementedError, match="solver budget.*= 7.*synchronous"):
        smb_rllib.SmbVectorEnv(cfg_of(), 2)
    assert closed == [1]


def test_pcgrl_vector_env_still_refuses_smb_and_points_here():
    from control_pcgrl_amd import PcgrlVectorEnv
    with pytest.raises(NotImplementedError, match="smb.*SmbVectorEnv"):
        PcgrlVectorEnv(cfg_of(), 2)


def test_make_vector_env_dispatches_on_the_problem(monkeypatch):
    import control_pcgrl_amd
    seen = []

    class FakeSmb:
        def __init__(self, cfg, num_envs, **kw):
            seen.append(("smb", num_envs, kw))

    class FakeEngine:
        def __init__(self, cfg, num_envs, **kw):
            seen.append(("engine", num_envs, kw))

    monkeypatch.setattr(smb_rllib, "SmbVectorEnv", FakeSmb)
    monkeypatch.setattr(rllib_env, "PcgrlVectorEnv", FakeEngine)
    assert control_pcgrl_amd.make_vector_env is smb_rllib.make_vector_env
    assert isinstance(smb_rllib.make_vector_env(cfg_of(), 20, obs_dtype=np.uint8), FakeSmb)
    assert seen[-1] == ("smb", 20, {"obs_dtype": np.uint8})
    assert isinstance(smb_rllib.make_vector_env({"task": {"problem": "smb"}, "num_envs_per_worker": 4}, 4), FakeSmb)
    assert isinstance(smb_rllib.make_vector_env(NS(task=NS(problem="binary")), 3, device="cuda:0"), FakeEngine)
    assert seen[-1] == ("engine", 3, {"device": "cuda:0"})


def test_the_adapters_share_one_bookkeeping():
    """the logic the two adapters share lives in one place, and both take RLlib's reset calls from it"""
    from control_pcgrl_amd import PcgrlVectorEnv, SmbVectorEnv
    for cls in (PcgrlVectorEnv, SmbVectorEnv):
        assert issubclass(cls, rllib_env._VectorAdapter)
        for name in ("vector_reset", "reset_at", "restart_at", "get_sub_environments", "try_render_at", "close", "set_trgs"):
            assert getattr(cls, name) is getattr(rllib_env._VectorAdapter, name), (cls, name)
        assert "vector_step" in vars(cls) and "_masked_reset" in vars(cls)


def test_the_driver_surface_of_the_env():
    for name in ("step_into", "observe_into", "observe_f32_into", "reset_masked", "stats_into"):
        assert callable(getattr(smb_env.SmbVecEnv, name)), name


def test_abi_null_handles():
    L = _lib.lib()
    assert L.pcgrl_smb_env_obs_f32_bytes(None) == -1
    buf = np.zeros(64, np.float32)
    assert L.pcgrl_smb_env_observe_f32(None, buf.ctypes.data, None) == 1  # PCGRL_EINVAL, before any HIP call
    assert b"pcgrl_smb_env_observe_f32" in L.pcgrl_last_error()
    assert L.pcgrl_smb_env_observe_f32(None, None, None) == 1


def test_the_new_unit_is_part_of_the_build():
    assert "smb/pcgrl_k_smb_vector.hip" in _lib.UNITS and "smb/pcgrl_smb_vector.h" in _lib.HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, "smb", "pcgrl_k_smb_vector.hip")) and os.path.exists(_lib.SMB_VECTOR_HEADER)
    assert set(_lib.SMB_VECTOR_SYMBOLS) == {"pcgrl_smb_env_obs_f32_bytes", "pcgrl_smb_env_observe_f32"}


# -- the numpy statement of the float32 image ---------------------------------------------------------------------------------
def test_statement_by_hand():
    """a 4 x 5 map seen from its corner (0, 0) through a 3 x 4 window with one control: rows -1..1, columns -2..1"""
    grid = np.arange(20, dtype=np.uint8).reshape(4, 5) % 7
    ctrl = [0.25, 0.5]
    im = V.f32_image(grid, (0, 0), (3, 4), ctrl)
    assert im.shape == (3, 4, 10) and im.dtype == np.float32
    assert (im[..., 0] == 0.25).all() and (im[..., 1] == 0.5).all()  # the planes come first, each constant over the window
    onehot = im[..., 2:]
    assert (onehot.sum(-1) == 1).all()
    ch = onehot.argmax(-1)
    assert ch[0].tolist() == [0, 0, 0, 0]  # map row -1
    assert ch[1].tolist() == [0, 0, 1 + 0, 1 + 1]  # map row 0: columns -2, -1 outside, then cells (0, 0) and (0, 1)
    assert ch[2].tolist() == [0, 0, 1 + 5, 1 + 6]  # map row 1: tiles 5 % 7 and 6 % 7


@pytest.mark.parametrize("shape,window", [((4, 5), (8, 10)), ((5, 7), (9, 13)), ((6, 12), (5, 9)), ((16, 116), (32, 232))])
def test_statement_equals_the_rules_observation(shape, window):
    """without controls the image is float32(one-hot) of the rules' observation, at every corner and in the middle"""
    H, W = shape
    rules = E.SmbEnvRules("turtle", shape, obs_window=window)
    rules.grid = sl.make("random", 5, H, W)
    ctrl = np.array([0.125, 3.5, -1.0, 0.0], np.float32)
    for pos in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
        rules.pos = list(pos)
        want = rules.observation()
        assert np.array_equal(V.f32_image(rules.grid, pos, window), want.astype(np.float32))
        im = V.f32_image(rules.grid, pos, window, ctrl)
        assert np.array_equal(im[..., 4:], want.astype(np.float32))
        assert np.array_equal(im[..., :4], np.broadcast_to(ctrl, window + (4,)))
    batch = V.f32_images(np.stack([rules.grid] * 2), [(0, 0), (1, 1)], window, np.stack([ctrl, ctrl + 1]))
    assert batch.shape == (2,) + window + (12,) and np.array_equal(batch[1][..., :4], np.broadcast_to(ctrl + 1, window + (4,)))
