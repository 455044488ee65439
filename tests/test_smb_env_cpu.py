"""Stepping Super Mario Bros environments, the part that needs no GPU: the fixtures of tests/golden/smb_env (recorded from the
reference by tools/gen_golden_smb_env.py) replay through the plain-Python rules of tests/smb_env_rules.py, the rules' search count
is resets plus solidity-changing edits, the ABI refuses bad arguments before any HIP call, every refusal of the Python layer
names its reason, and make_env / make_vec_env dispatch on the problem."""
import ctypes as C
import glob
import os
import sys
import zlib
from types import SimpleNamespace as NS

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smb_env_rules as E  # noqa: E402
import smb_rules as R  # noqa: E402

from control_pcgrl_amd import _lib, problems, smb, smb_env  # noqa: E402
from control_pcgrl_amd.vec_env import build_config  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smb_env")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
EXPECTED = ["narrow_16x116", "narrow_16x127", "narrow_4x5", "narrow_6x12_win5x9", "narrow_8x20_p300", "paint_6x70_p300",
            "paint_8x30_p300", "turtle_16x116", "turtle_5x7_alt", "turtle_5x7_cp02", "turtle_8x20_p300"]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes()) & 0xFFFFFFFF


def rules_of(z):
    cp = float(z["change_percentage"])
    weights = {k: float(w) for k, w in zip(R.STAT_KEYS, z["weights"])}
    return E.SmbEnvRules(str(z["representation"]), tuple(int(s) for s in z["map_shape"]), seed=int(z["seed"]),
                         obs_window=tuple(int(s) for s in z["obs_window"]), weights=weights,
                         change_percentage=None if cp < 0 else cp, solver_power=int(z["solver_power"]))


def test_the_fixture_set_is_complete():
    assert FIXTURES == EXPECTED
    total = 0
    for name in FIXTURES:
        size = os.path.getsize(os.path.join(GOLDEN, name + ".npz"))
        assert size <= 100 * 1024, name
        total += size
    assert total <= 400 * 1024


@pytest.mark.parametrize("name", EXPECTED)
def test_fixture_replays_through_the_rules(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert list(z["stat_keys"]) == R.STAT_KEYS
    rules = rules_of(z)
    assert (rules.max_iterations, -1 if rules.max_changes is None else rules.max_changes) == \
        (int(z["max_iterations"]), int(z["max_changes"]))
    full = {int(t): k for k, t in enumerate(z["full_steps"])}
    ob = rules.reset()
    assert crc(ob) == int(z["obs0_crc"]) and rules.pos == list(z["pos0"]) and rules.stats == list(z["stats0"])
    assert np.array_equal(ob, z["full_obs"][full[-1]]) and np.array_equal(rules.grid, z["full_map"][full[-1]])
    expected_searches = 1
    for t, a in enumerate(z["actions"]):
        ob, rew, done, info = rules.step(int(a), auto_reset=True)
        expected_searches += int(info["searched"]) + int(done)
        stats = info["final_stats"] if done else info["stats"]
        assert stats == list(z["stats"][t]) and rew == float(z["reward"][t]) and done == bool(z["done"][t]), (name, t)
        assert (info["iteration"], info["changes"]) == (int(z["iteration"][t]), int(z["changes"][t])), (name, t)
        assert rules.pos == list(z["pos"][t]) and crc(ob) == int(z["obs_crc"][t]), (name, t)
        if t in full:
            assert np.array_equal(ob, z["full_obs"][full[t]]) and np.array_equal(rules.grid, z["full_map"][full[t]]), (name, t)
    # the two shortcuts as a count: a search per reset and per edit that changed a cell's solidity, and no other
    assert rules.searches == expected_searches
    solid = np.isin(np.arange(7), R.BLOCKING)
    assert list(np.nonzero(solid)[0]) == [1, 3, 4, 6]


def test_search_count_on_a_painted_level():
    """painting a level cell by cell searches exactly where the solidity of the cell changes"""
    rules = E.SmbEnvRules("narrow", (4, 5), seed=3, solver_power=300)
    rules.reset()
    before = rules.grid.copy()
    level = np.array([[0, 0, 5, 0, 0], [0, 2, 0, 0, 6], [1, 1, 0, 3, 1], [1, 1, 0, 1, 4]], np.uint8)
    actions = [int(level[0, 0])] + [int(t) for t in level.ravel()]
    cur, want = before.copy().ravel(), 1
    cells = [0] + list(range(20))
    for c, a in zip(cells, actions):
        want += int(E.is_solid(cur[c]) != E.is_solid(a))
        cur[c] = a
        rules.step(a)
    assert np.array_equal(rules.grid, level) and rules.searches == want
    assert rules.stats == R.get_stats(level, 300)[0]  # the kept play statistics are those of a full evaluation


def test_lib_lists_the_unit_the_header_and_the_symbols():
    assert "smb/pcgrl_k_smb_env.hip" in _lib.UNITS and "smb/pcgrl_smb_env.h" in _lib.HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, "smb", "pcgrl_k_smb_env.hip")) and os.path.exists(_lib.SMB_ENV_HEADER)
    header = open(_lib.SMB_ENV_HEADER).read()
    import re
    declared = set(re.findall(r"\b(pcgrl_smb_env_\w+)\(", header))
    assert set(_lib.SMB_ENV_SYMBOLS) == declared
    assert not declared & (set(_lib.SYMBOLS) | set(_lib.SMB_SYMBOLS))
    L = _lib.lib()
    for name, (res, args) in _lib.SMB_ENV_SYMBOLS.items():
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype == res, name
        params = re.search(name + r"\(([^;]*)\);", header, re.S).group(1)
        assert len(params.split(",")) == len(args), name
    assert C.sizeof(_lib.PcgrlSmbEnvConfig) == 9 * 4 + 36 + 3 * 72


def env_cfg(shape=(16, 116), rep=0, window=None, power=10000, n=4):
    base = smb.smb_config(shape, power)
    cfg = _lib.PcgrlSmbEnvConfig()
    cfg.h, cfg.w, cfg.representation = shape[0], shape[1], rep
    cfg.obs_window[0], cfg.obs_window[1] = window if window is not None else (2 * shape[0], 2 * shape[1])
    cfg.max_iterations, cfg.max_changes, cfg.solver_power, cfg.n_envs = shape[0] * shape[1] * 3 + 1, -1, power, n
    for i in range(9):
        cfg.has_trg[i], cfg.weight[i], cfg.trg_lo[i], cfg.trg_hi[i] = base.has_trg[i], base.weight[i], base.trg_lo[i], base.trg_hi[i]
    return cfg


def test_abi_argument_checks_need_no_device():
    L = _lib.lib()
    EINVAL, EUNSUPPORTED = 1, 2
    ok = env_cfg()
    assert L.pcgrl_smb_env_workspace_bytes(C.byref(ok)) == 4 * L.pcgrl_smb_workspace_bytes(1, 16, 116, 10000)
    assert L.pcgrl_smb_env_obs_bytes(C.byref(ok)) == 32 * 232 * 8 == 59392
    assert L.pcgrl_smb_env_workspace_bytes(None) == -1 and L.pcgrl_smb_env_obs_bytes(None) == -1
    need = L.pcgrl_smb_env_workspace_bytes(C.byref(ok))
    out = C.c_void_p()

    def create(cfg, ws=0x1000, wb=need, o=out):
        return L.pcgrl_smb_env_create(C.byref(cfg) if cfg is not None else None, 0, ws, wb, C.byref(o) if o is not None else None)

    # pointers that are never dereferenced: every call below is refused before any HIP call
    assert create(None) == EINVAL and create(ok, o=None) == EINVAL
    assert create(ok, ws=None) == EINVAL and create(ok, wb=need - 1) == EINVAL and create(ok, ws=0x1004) == EINVAL
    assert b"workspace" in L.pcgrl_last_error()
    assert create(env_cfg(n=0)) == EINVAL and create(env_cfg(rep=3)) == EINVAL
    for bad in (env_cfg((3, 116)), env_cfg((17, 116)), env_cfg((16, 129)), env_cfg((16, 0)), env_cfg(power=0),
                env_cfg(power=16001)):
        assert create(bad) == EUNSUPPORTED and L.pcgrl_smb_env_workspace_bytes(C.byref(bad)) == -1
    assert create(env_cfg(rep=2)) == EUNSUPPORTED and b"wide" in L.pcgrl_last_error()
    for window in ((256, 20), (20, 256), (0, 20), (20, 0), (32, 256)):
        assert create(env_cfg((16, 128), window=window)) == EUNSUPPORTED, window
    assert b"obs_window" in L.pcgrl_last_error()
    assert L.pcgrl_smb_env_workspace_bytes(C.byref(env_cfg((16, 127)))) > 0  # the default window of 16 x 127 is 254 wide
    assert L.pcgrl_smb_env_workspace_bytes(C.byref(env_cfg((16, 128)))) == -1  # ... and 16 x 128's is 256
    assert L.pcgrl_smb_env_workspace_bytes(C.byref(env_cfg((16, 128), window=(32, 255)))) > 0
    assert out.value is None
    # a null handle, everywhere
    assert L.pcgrl_smb_env_seed(None, None) == EINVAL and L.pcgrl_smb_env_reset(None, None, None, None, None, None) == EINVAL
    assert L.pcgrl_smb_env_step(None, None, 1, None, None, None, None, None, None) == EINVAL
    assert L.pcgrl_smb_env_observe(None, None, None) == EINVAL and L.pcgrl_smb_env_poll_error(None) == EINVAL
    assert L.pcgrl_smb_env_get_state(None, *([None] * 8)) == EINVAL
    assert L.pcgrl_smb_env_get_last_episode(None, *([None] * 5)) == EINVAL
    L.pcgrl_smb_env_destroy(None)


def cfg_of(rep="narrow", shape=(16, 116), **kw):
    task = NS(name="smb", problem="smb", map_shape=shape, obs_window=kw.pop("obs_window", None), weights=None, controls=None)
    base = dict(representation=rep, task=task, controls=None, change_percentage=None, max_board_scans=3, n_aux_tiles=0,
                static_prob=None, n_static_walls=None, act_window=None, show_agents=False,
                multiagent=NS(n_agents=0, policies="centralized"))
    base.update(kw)
    return NS(**base)


def test_every_refusal_names_its_reason():
    from control_pcgrl_amd import PcgrlVectorEnv, make_env, make_vec_env

    def refused(match, fn, *a, **kw):
        with pytest.raises(NotImplementedError, match=match):
            fn(*a, **kw)

    refused("wide", make_vec_env, cfg_of("wide"), 2)
    refused("wide", smb_env.SmbVecEnv, "wide", (16, 116), 2)
    refused("obs_window.*255", make_vec_env, cfg_of(obs_window=(32, 256)), 2)
    refused("obs_window.*255", make_vec_env, cfg_of(shape=(16, 128)), 2)  # the default window of 16 x 128
    refused("controls", make_vec_env, cfg_of(controls=["enemies"]), 2)
    refused("static tiles", make_vec_env, cfg_of(static_prob=0.1), 2)
    refused("static tiles", make_vec_env, cfg_of(n_static_walls=2), 2)
    refused("act_window", make_vec_env, cfg_of(act_window=(3, 3)), 2)
    refused("multiagent", make_vec_env, cfg_of("turtle", multiagent=NS(n_agents=2, policies="centralized")), 2)
    refused("codes", make_vec_env, cfg_of(obs_format="codes"), 2)
    refused("sub_batches", make_vec_env, cfg_of(), 4, sub_batches=2)
    refused("smb", PcgrlVectorEnv, cfg_of(), 2)
    refused("wide", make_env, cfg_of("wide"))
    refused("outside 4..16", smb_env.SmbVecEnv, "narrow", (3, 116), 2)
    refused("outside 4..16", smb_env.SmbVecEnv, "narrow", (16, 116), 2, solver_power=16001)
    for name in ("set_solver_budget", "step_ready"):
        with pytest.raises(NotImplementedError, match="resumable"):
            getattr(smb_env.SmbVecEnv, name)(None, 1)
    with pytest.raises(ValueError):
        smb_env.SmbVecEnv("cellular", (16, 116), 2)


def test_dispatch_reaches_the_smb_env(monkeypatch):
    """make_vec_env / make_env hand an smb cfg to smb_env before build_config sees it"""
    from control_pcgrl_amd import make_env, make_vec_env
    seen = []

    class Fake:
        def __init__(self, representation, map_shape, num_envs, **kw):
            seen.append((representation, tuple(map_shape), num_envs, kw))
            self.num_envs, self.auto_reset = num_envs, kw["auto_reset"]
            self.obs_shape, self.num_actions, self.weights = (8, 10, 8), 7, {}
            self.spec = smb.smb_spec(map_shape)

    monkeypatch.setattr(smb_env, "SmbVecEnv", Fake)
    v = make_vec_env(cfg_of("turtle", (8, 20), obs_window=(5, 9), change_percentage=0.2), 3, seeds=[1, 2, 3])
    assert isinstance(v, Fake)
    rep, shape, n, kw = seen[-1]
    assert (rep, shape, n) == ("turtle", (8, 20), 3) and kw["obs_window"] == (5, 9) and kw["change_percentage"] == 0.2
    assert kw["seeds"] == [1, 2, 3] and kw["auto_reset"] is True and kw["solver_power"] == 10000
    e = make_env(cfg_of("narrow", (4, 5)))
    assert isinstance(e, smb_env.SmbGymEnv) and seen[-1][:3] == ("narrow", (4, 5), 1) and seen[-1][3]["auto_reset"] is False
    assert e.action_space.n == 7 and e.observation_space.shape == (8, 10, 8)


def test_stepping_smb_stays_outside_the_engine():
    """the three facts tests/test_smb_cpu.py pins: smb is an env class of its own, the 2-D engine still does not know it"""
    assert "smb" not in problems.PROBLEMS
    with pytest.raises(ValueError):
        problems.problem_spec("smb", (16, 116))
    with pytest.raises(ValueError):
        build_config("smb", "narrow", (16, 116))
