"""Controllable generation for Super Mario Bros environments, the part that needs no GPU: the fixtures of
tests/golden/smb_ctrl (recorded from the reference by tools/gen_golden_smb_ctrl.py) replay through the plain-Python rules of
tests/smb_ctrl_rules.py, the host restatement of the resampled targets against the documented formula, the refusals of the
Python layer and of the C ABI (raised before any HIP call), and the make_vec_env / make_env dispatch."""
import ctypes as C
import json
import os
import re
import sys
import zlib
from types import SimpleNamespace as NS

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smb_ctrl_rules as CR  # noqa: E402
import smb_rules as R  # noqa: E402

from control_pcgrl_amd import _lib, smb, smb_env  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smb_ctrl")
FIXTURES = ["narrow_4x5_jumps_sol", "turtle_5x7_cp02_tuple", "paint_8x20_sol", "narrow_4x5_all9"]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes()) & 0xFFFFFFFF


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cp = float(z["change_percentage"])
    kw = dict(representation=str(z["representation"]), map_shape=tuple(int(s) for s in z["map_shape"]),
              weights={k: float(w) for k, w in zip(R.STAT_KEYS, z["weights"])}, change_percentage=None if cp < 0 else cp,
              solver_power=int(z["solver_power"]))
    events = {}
    for t, trgs in json.loads(str(z["events"])):
        events.setdefault(int(t), []).append({k: tuple(v) if isinstance(v, list) else v for k, v in trgs.items()})
    return z, kw, [str(k) for k in z["controls"]], events


@pytest.mark.parametrize("name", FIXTURES)
def test_rules_replay_the_fixture(name):
    z, kw, controls, events = load(name)
    rules = CR.SmbCtrlRules(kw["representation"], kw["map_shape"], controls, seed=int(z["seed"]), weights=kw["weights"],
                            change_percentage=kw["change_percentage"], solver_power=kw["solver_power"])
    for trgs in events.get(-1, []):
        rules.set_trgs(trgs)
    ob = rules.reset()
    assert crc(ob) == int(z["obs0_crc"]) and rules.stats == z["stats0"].tolist() and rules.ctrl_obs() == z["ctrl0"].tolist()
    resets = {int(t): r for r, t in enumerate(z["reset_at"])}

    def targets_in_force(r):
        assert [rules.trg[k][0] for k in R.STAT_KEYS] == z["reset_lo"][r].tolist()
        assert [rules.trg[k][1] for k in R.STAT_KEYS] == z["reset_hi"][r].tolist()
        assert [rules.shown[k] for k in controls] == z["reset_shown"][r].tolist()

    targets_in_force(0)
    for t, a in enumerate(z["actions"]):
        for trgs in events.get(t, []):
            rules.set_trgs(trgs)
        ob, rew, done, info = rules.step(int(a), auto_reset=True)
        assert done == bool(z["done"][t]) and crc(ob) == int(z["obs_crc"][t]), t
        assert (info["final_stats"] if done else info["stats"]) == z["stats"][t].tolist(), t
        assert rules.ctrl_obs() == z["ctrl"][t].tolist(), t  # exact: the same two divisions in double
        want = float(z["reward"][t])
        assert rew == want if z["dyadic"][t] else abs(rew - want) <= 1e-9, (t, rew, want)
        if done:
            targets_in_force(resets[t])
    assert len(resets) == 1 + int(z["done"].sum())


def test_the_fixtures_show_their_cases():
    seen = set()
    for name in FIXTURES:
        z, kw, controls, events = load(name)
        seen.add("non-integer reward" if np.any(z["reward"] != np.round(z["reward"])) else "")
        seen.add("both kinds of step" if 0 < z["dyadic"].sum() < len(z["dyadic"]) else "")
        seen.add("tuple" if any(isinstance(v, tuple) for ev in events.values() for trgs in ev for v in trgs.values()) else "")
        seen.add("all nine" if len(controls) == 9 else "")
        seen.add("done by changes" if kw["change_percentage"] is not None and z["done"].any() else "")
        seen.add("done by iterations" if kw["change_percentage"] is None and z["done"].any() else "")
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= 16 * 1024
    assert {"non-integer reward", "both kinds of step", "tuple", "all nine", "done by changes", "done by iterations"} <= seen


def test_resampled_targets_follow_the_documented_formula():
    """u * (hi - lo) + lo, u the top 53 bits of mix64(mix64(seed + c * G) ^ (env * A + (j + 1) * B)): an independent numpy uint64
    version, and three values worked out once by hand from that formula"""
    def mix(z):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return z ^ (z >> np.uint64(31))

    def numpy_version(seed, env, c, j, lo, hi):
        with np.errstate(over="ignore"):
            a = mix(np.uint64(seed) + np.uint64(c) * np.uint64(0x9e3779b97f4a7c15))
            b = np.uint64(env) * np.uint64(0xd1b54a32d192ed03) + np.uint64(j + 1) * np.uint64(0x8cb92ba72f3d8dd7)
            r = mix(a ^ b)
        return float(r >> np.uint64(11)) * (1.0 / 9007199254740992.0) * (hi - lo) + lo

    rng = np.random.default_rng(5)
    for _ in range(300):
        seed, env, c, j = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 31)), int(rng.integers(0, 2 ** 32)), \
            int(rng.integers(0, 9))
        lo, hi = float(rng.random() * 10), float(10 + rng.random() * 2000)
        t = CR.trg_resampled(seed, env, c, j, lo, hi)
        assert t == numpy_version(seed, env, c, j, lo, hi) and lo <= t < hi
    assert CR.mix64(0) == 0 and CR.mix64(1) == 0x5692161d100b05e5  # splitmix64's finaliser
    assert CR.trg_resampled(0, 0, 0, 0, 0.0, 1.0) == float(CR.mix64(0x8cb92ba72f3d8dd7) >> 11) / 2.0 ** 53
    assert CR.trg_resampled(7, 3, 2, 1, 0.0, 116.0) == numpy_version(7, 3, 2, 1, 0.0, 116.0)
    # the draws of one env differ from counter to counter and from control to control
    assert len({CR.trg_resampled(9, 4, c, j, 0.0, 1.0) for c in range(4) for j in range(3)}) == 12


def test_lib_lists_the_header_and_the_symbols():
    assert "smb/pcgrl_smb_ctrl.h" in _lib.HEADERS and os.path.exists(_lib.SMB_CTRL_HEADER)
    header = open(_lib.SMB_CTRL_HEADER).read()
    declared = set(re.findall(r"\b(pcgrl_smb_ctrl_\w+)\(", header))
    assert set(_lib.SMB_CTRL_SYMBOLS) == declared
    L = _lib.lib()
    for name, (res, args) in _lib.SMB_CTRL_SYMBOLS.items():
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype == res, name
        params = re.search(r"\b" + name + r"\(([^;]*)\);", header, re.S).group(1)
        assert len(params.split(",")) == len(args), name
    # the existing entry points keep their signatures
    assert len(_lib.SMB_ENV_SYMBOLS["pcgrl_smb_env_step"][1]) == 9 and len(_lib.SMB_ENV_SYMBOLS["pcgrl_smb_env_reset"][1]) == 6


def test_abi_refusals_need_no_device():
    L = _lib.lib()
    EINVAL = 1
    idx, rng = (C.c_int32 * 2)(5, 8), (C.c_double * 2)(116.0, 348.0)
    assert L.pcgrl_smb_ctrl_attach(None, 2, idx, rng, rng, None) == EINVAL and b"null handle" in L.pcgrl_last_error()
    assert L.pcgrl_smb_ctrl_count(None) == -1
    assert L.pcgrl_smb_ctrl_queue(None, None, 1, idx, None, None, None, None) == EINVAL
    assert L.pcgrl_smb_ctrl_observe(None, None, None) == EINVAL
    assert L.pcgrl_smb_ctrl_set_resampling(None, 1, 0, rng, rng, None) == EINVAL
    assert L.pcgrl_smb_ctrl_get(None, None, None, None, None, None) == EINVAL


def test_python_refusals_come_before_any_device_call():
    with pytest.raises(ValueError, match="not an smb statistic"):
        smb_env.SmbVecEnv("narrow", (4, 5), 2, controls=["path-length"])
    with pytest.raises(ValueError, match="twice"):
        smb_env.SmbVecEnv("narrow", (4, 5), 2, controls=["jumps", "jumps"])
    bare = smb_env.SmbVecEnv.__new__(smb_env.SmbVecEnv)  # no handle: the checks below come first
    bare._h, bare.controls, bare.num_envs = None, [], 2
    for call in (lambda: bare.queue_targets({"jumps": 3.0}), bare.sample_uniform_targets, bare.set_target_resampling,
                 bare.get_targets):
        with pytest.raises(ValueError, match="without `controls`"):
            call()
    bare.controls = ["jumps"]
    bare.device = "cpu"
    with pytest.raises(ValueError, match="not a control metric"):
        bare.queue_targets({"enemies": 3.0})
    with pytest.raises(ValueError, match="whole-number lo"):
        bare.queue_targets({"jumps": (2.5, 5)})
    with pytest.raises(ValueError, match="at least one"):
        bare.queue_targets({})


def cfg_of(rep="narrow", shape=(4, 5), **kw):
    task = NS(name="smb", problem="smb", map_shape=shape, obs_window=None, weights=None, controls=None,
              alp_gmm=kw.pop("alp_gmm", False))
    base = dict(representation=rep, task=task, controls=None, change_percentage=None, max_board_scans=3, n_aux_tiles=0,
                static_prob=None, n_static_walls=None, act_window=None, show_agents=False,
                multiagent=NS(n_agents=0, policies="centralized"), evaluate=True)
    base.update(kw)
    return NS(**base)


def test_dispatch_hands_the_controls_on(monkeypatch):
    import torch
    from control_pcgrl_amd import make_env, make_vec_env
    seen = []

    class Fake:
        def __init__(self, representation, map_shape, num_envs, **kw):
            seen.append((representation, tuple(map_shape), num_envs, kw))
            self.num_envs, self.auto_reset = num_envs, kw["auto_reset"]
            self.obs_shape, self.num_actions, self.weights = (8, 10, 8), 7, {}
            self.spec = smb.smb_spec(map_shape)
            self.controls = list(kw.get("controls") or [])

    monkeypatch.setattr(smb_env, "SmbVecEnv", Fake)
    v = make_vec_env(cfg_of(controls=["jumps", "sol-length"]), 3, seeds=[1, 2, 3])
    assert isinstance(v, Fake) and seen[-1][3]["controls"] == ["jumps", "sol-length"]
    assert seen[-1][3]["reward_dtype"] == torch.float64  # as make_vec_env does for the 2-D engine
    make_vec_env(cfg_of(), 3)
    assert "controls" not in seen[-1][3] and seen[-1][3]["reward_dtype"] == torch.float32
    e = make_env(cfg_of(controls=["enemies", "empty", "dist-win"]))
    assert isinstance(e, smb_env.SmbGymEnv) and e.ctrl_metrics == ["enemies", "empty", "dist-win"]
    assert e.observation_space.shape == (8, 10, 8 + 6) and e.cond_bounds["jumps"] == (0, 116)
    assert e.metric_trgs["empty"] == (900, 1856) and hasattr(e, "set_trgs")
    e = make_env(cfg_of())
    assert e.ctrl_metrics == [] and e.observation_space.shape == (8, 10, 8)
    # without cfg.evaluate the reference puts a target sampler on top (rl/envs.py:70-76): refused, by name
    with pytest.raises(NotImplementedError, match="alp_gmm"):
        make_vec_env(cfg_of(controls=["jumps"], alp_gmm=True, evaluate=False), 2)
    with pytest.raises(NotImplementedError, match="controls without cfg.evaluate.*UniformNoiseyTargets"):
        make_vec_env(cfg_of(controls=["jumps"], evaluate=False), 2)
    n_seen = len(seen)
    with pytest.raises(NotImplementedError, match="controls without cfg.evaluate"):
        make_env(cfg_of(controls=["jumps"], evaluate=None))
    assert len(seen) == n_seen  # refused before any env is made
    make_vec_env(cfg_of(evaluate=False), 2)  # no controls: cfg.evaluate does not matter
    # what stays refused, by name
    for match, cfg in (("static tiles", cfg_of(controls=["jumps"], static_prob=0.1)), ("act_window", cfg_of(act_window=(3, 3))),
                       ("wide", cfg_of("wide", controls=["jumps"])), ("codes", cfg_of(obs_format="codes"))):
        with pytest.raises(NotImplementedError, match=match):
            make_vec_env(cfg, 2)
    with pytest.raises(NotImplementedError, match="sub_batches"):
        make_vec_env(cfg_of(controls=["jumps"]), 4, sub_batches=2)


def test_rules_targets_start_static_and_a_requeue_replaces():
    rules = CR.SmbCtrlRules("narrow", (4, 5), ["jumps", "sol-length"], seed=3, solver_power=300)
    assert rules.trg["empty"] == (900.0, 1855.0) and rules.trg["jumps"] == (20.0, 1855.0) and rules.shown["jumps"] == 938.0
    rules.set_trgs({"jumps": 7.5})
    rules.set_trgs({"sol-length": (3, 6)})  # the queue is replaced, not merged
    rules.reset()
    assert rules.trg["jumps"] == (20.0, 1855.0) and rules.trg["sol-length"] == (3.0, 5.0) and rules.shown["sol-length"] == 4.5
    rules.reset()  # nothing queued: the targets stay
    assert rules.trg["sol-length"] == (3.0, 5.0)
    rules.set_resampling(True, seed=11)
    rules.set_trgs({"jumps": 1.0})
    rules.reset()
    assert rules.trg["jumps"][0] == CR.trg_resampled(11, 0, 0, 0, 0, 116) and rules.draws == 1 and rules.queue is None
