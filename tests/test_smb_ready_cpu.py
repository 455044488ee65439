"""Asynchronous stepping of Super Mario Bros environments, the part that needs no GPU: the ABI's header, symbol table and unit,
its refusals before any HIP call, the dispatch on cfg.task.solver_budget, and the launch rules of tests/smb_ready_rules.py
replaying the fixtures of tests/golden/smb_env at several budgets -- the emitted transitions are the fixture's in order, and
the number of launches is what the search lengths T give."""
import ctypes as C
import os
import re
import sys
import zlib
from types import SimpleNamespace as NS

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smb_env_rules as E  # noqa: E402
import smb_ready_rules as RR  # noqa: E402
import smb_rules as R  # noqa: E402

from control_pcgrl_amd import _lib, smb, smb_env, smb_ready  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smb_env")
EINVAL = 1


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes()) & 0xFFFFFFFF


def test_lib_lists_the_unit_the_header_and_the_symbols():
    assert "smb/pcgrl_k_smb_ready.hip" in _lib.UNITS and "smb/pcgrl_smb_ready.h" in _lib.HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, "smb", "pcgrl_k_smb_ready.hip")) and os.path.exists(_lib.SMB_READY_HEADER)
    header = open(_lib.SMB_READY_HEADER).read()
    declared = set(re.findall(r"\b(pcgrl_smb_ready_\w+)\(", header))
    assert set(_lib.SMB_READY_SYMBOLS) == declared and len(declared) == 5
    assert not declared & (set(_lib.SYMBOLS) | set(_lib.SMB_SYMBOLS) | set(_lib.SMB_ENV_SYMBOLS))
    L = _lib.lib()
    for name, (res, args) in _lib.SMB_READY_SYMBOLS.items():
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype == res, name
        params = re.search(name + r"\(([^;]*)\);", header, re.S).group(1)
        assert len(params.split(",")) == len(args), name
    # the status bits are pcgrl_amd.h's: the new header defines none
    assert "PCGRL_ENV_EMITTED =" not in header and re.search(r"PCGRL_ENV_EMITTED = 1, PCGRL_ENV_BUSY = 2", open(_lib.HEADER).read())
    assert (smb_ready.STATUS_EMITTED, smb_ready.STATUS_BUSY) == (RR.EMITTED, RR.BUSY) == (1, 2)


def env_cfg(shape=(16, 116), rep=0, power=10000, n=4):
    base = smb.smb_config(shape, power)
    cfg = _lib.PcgrlSmbEnvConfig()
    cfg.h, cfg.w, cfg.representation = shape[0], shape[1], rep
    cfg.obs_window[0], cfg.obs_window[1] = 2 * shape[0], 2 * shape[1]
    cfg.max_iterations, cfg.max_changes, cfg.solver_power, cfg.n_envs = shape[0] * shape[1] * 3 + 1, -1, power, n
    for i in range(9):
        cfg.has_trg[i], cfg.weight[i], cfg.trg_lo[i], cfg.trg_hi[i] = base.has_trg[i], base.weight[i], base.trg_lo[i], base.trg_hi[i]
    return cfg


def test_abi_argument_checks_need_no_device():
    L = _lib.lib()
    # a null handle, everywhere: refused before any HIP call
    assert L.pcgrl_smb_ready_set_budget(None, 16) == EINVAL and b"null handle" in L.pcgrl_last_error()
    assert L.pcgrl_smb_ready_set_budget(None, 0) == EINVAL and L.pcgrl_smb_ready_set_budget(None, -1) == EINVAL
    assert L.pcgrl_smb_ready_get_budget(None) == -1
    assert L.pcgrl_smb_ready_step(None, None, 1, None, None, None, None, None, None, None) == EINVAL
    assert L.pcgrl_smb_ready_step(None, 0x1000, 1, 0x1000, None, None, None, None, 0x1000, None) == EINVAL
    assert L.pcgrl_smb_ready_busy(None, None, None) == EINVAL and L.pcgrl_smb_ready_busy(None, 0x1000, None) == EINVAL
    # the park record: the loop's words, the mode and the action, and the visited set of 134 * 21 * 6 bits
    seen_words = (134 * 21 * 6 + 31) // 32
    assert seen_words * 4 == 2112
    park = L.pcgrl_smb_ready_park_bytes(C.byref(env_cfg()))
    assert park == 48 + 2112 and park % 16 == 0
    assert park == L.pcgrl_smb_ready_park_bytes(C.byref(env_cfg((4, 5), rep=1, power=1, n=1)))  # whatever the shape
    assert L.pcgrl_smb_ready_park_bytes(None) == -1
    for bad in (env_cfg((3, 116)), env_cfg((16, 129)), env_cfg(power=16001), env_cfg(rep=2), env_cfg(n=0)):
        assert L.pcgrl_smb_ready_park_bytes(C.byref(bad)) == -1


def cfg_of(rep="narrow", shape=(16, 116), **task_kw):
    task = NS(name="smb", problem="smb", map_shape=shape, obs_window=None, weights=None, controls=None, **task_kw)
    return NS(representation=rep, task=task, controls=None, change_percentage=None, max_board_scans=3, n_aux_tiles=0,
              static_prob=None, n_static_walls=None, act_window=None, show_agents=False,
              multiagent=NS(n_agents=0, policies="centralized"))


def test_dispatch_on_the_solver_budget(monkeypatch):
    from control_pcgrl_amd import SmbReadyVecEnv, make_vec_env
    assert SmbReadyVecEnv is smb_ready.SmbReadyVecEnv and issubclass(SmbReadyVecEnv, smb_env.SmbVecEnv)
    seen = []

    def fake(tag):
        class Fake:
            def __init__(self, representation, map_shape, num_envs, **kw):
                seen.append((tag, representation, tuple(map_shape), num_envs, kw))
        return Fake

    monkeypatch.setattr(smb_env, "SmbVecEnv", fake("sync"))
    monkeypatch.setattr(smb_ready, "SmbReadyVecEnv", fake("ready"))
    make_vec_env(cfg_of("turtle", (8, 20), solver_budget=64, solver_power=300), 3, seeds=[1, 2, 3])
    tag, rep, shape, n, kw = seen[-1]
    assert (tag, rep, shape, n) == ("ready", "turtle", (8, 20), 3) and kw["solver_budget"] == 64 and kw["solver_power"] == 300
    assert kw["seeds"] == [1, 2, 3] and kw["auto_reset"] is True
    for cfg in (cfg_of(), cfg_of(solver_budget=0), cfg_of(solver_budget=None)):  # absent or 0: synchronous, as before
        make_vec_env(cfg, 2)
        assert seen[-1][0] == "sync" and "solver_budget" not in seen[-1][4]
    smb_env.make_smb_vec_env(cfg_of(solver_budget=1), 2)
    assert seen[-1][0] == "ready" and seen[-1][4]["solver_budget"] == 1
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="solver_budget"):
            make_vec_env(cfg_of(solver_budget=bad), 2)
    # everything make_smb_vec_env refuses is refused with a budget too
    with pytest.raises(NotImplementedError, match="wide"):
        make_vec_env(cfg_of("wide", solver_budget=8), 2)
    with pytest.raises(NotImplementedError, match="sub_batches"):
        make_vec_env(cfg_of(solver_budget=8), 4, sub_batches=2)


def test_the_python_layer_refuses_by_name():
    with pytest.raises(ValueError, match="solver_budget"):
        smb_ready.SmbReadyVecEnv("narrow", (4, 5), 2, solver_budget=0)
    for name in ("set_solver_budget", "step_ready"):  # the synchronous class points at this one
        with pytest.raises(NotImplementedError, match="resumable.*SmbReadyVecEnv"):
            getattr(smb_env.SmbVecEnv, name)(None, 1)


# ------------------------------------------------------------------------------------------------ the launch rules on fixtures

def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cp = float(z["change_percentage"])
    kw = dict(representation=str(z["representation"]), shape=tuple(int(s) for s in z["map_shape"]), seed=int(z["seed"]),
              obs_window=tuple(int(s) for s in z["obs_window"]), weights={k: float(w) for k, w in zip(R.STAT_KEYS, z["weights"])},
              change_percentage=None if cp < 0 else cp, solver_power=int(z["solver_power"]))
    return z, kw


_SEARCHES = {}


def searches_of(name):
    """(T0, [(T1, ended, T2)]) of a fixture through the synchronous rules: the reset's search, and per step its own search (0
    without one) and the next episode's where the step ended one"""
    if name not in _SEARCHES:
        z, kw = load(name)
        rules = E.SmbEnvRules(**kw)
        rules.reset()
        t0, steps = RR.search_length(rules), []
        for a in z["actions"]:
            _, _, done, info = rules.step(int(a), auto_reset=False)
            t1 = RR.search_length(rules) if info["searched"] else 0
            t2 = 0
            if done:
                rules.reset()
                t2 = RR.search_length(rules)
            steps.append((t1, bool(done), t2))
        _SEARCHES[name] = (t0, steps)
    return _SEARCHES[name]


def launches_from_lengths(t0, steps, B):
    """the launches the fixture's steps take at budget B, from the search lengths alone (the reset launch not counted)"""
    ceil = lambda a: -(-a // B)  # noqa: E731
    total = ceil(max(t0 - B, 0))  # the reset's statistics, where the reset launch did not finish them
    for t1, ended, t2 in steps:
        n = max(ceil(t1), 1)
        total += n + (ceil(max(t2 - (n * B - t1), 0)) if ended else 0)
    return total


def replay(name, B):
    """the fixture through the launch rules at budget B -> (launches, busy launches, the rules)"""
    z, kw = load(name)
    r = RR.SmbReadyRules(**kw)
    busy = r.reset(B)
    assert crc(r.observation()) == int(z["obs0_crc"])
    t, launches, busy_launches = 0, 0, 0
    actions = z["actions"]
    while t < len(actions):
        was_busy = r.busy()
        assert was_busy == busy
        status, out = r.launch(int(actions[t]) if not was_busy else -7, B)  # a busy env's action row is not looked at
        launches += 1
        busy = bool(status & RR.BUSY)
        busy_launches += int(busy)
        assert (out is not None) == bool(status & RR.EMITTED)
        if out is None:
            continue
        assert out["stats"] == z["stats"][t].tolist() and out["reward"] == float(z["reward"][t]), (name, B, t)
        assert out["done"] == bool(z["done"][t]) and out["pos"] == z["pos"][t].tolist(), (name, B, t)
        assert (out["iteration"], out["changes"]) == (int(z["iteration"][t]), int(z["changes"][t])), (name, B, t)
        assert crc(out["obs"]) == int(z["obs_crc"][t]), (name, B, t)
        t += 1
    while r.busy():  # the last episode's statistics
        status, out = r.launch(-7, B)
        launches += 1
        assert out is None
    assert not r.error
    return launches, busy_launches, r


CASES = [("narrow_4x5", (1, 5, 16, 64)), ("turtle_5x7_cp02", (7, 32, 200)), ("narrow_8x20_p300", (64, 1000)),
         ("paint_8x30_p300", (100,))]


@pytest.mark.parametrize("name,budgets", CASES)
def test_fixture_replays_through_the_launch_rules(name, budgets):
    t0, steps = searches_of(name)
    longest = max([t0] + [max(t1, t2) for t1, _, t2 in steps])
    for B in budgets:
        launches, busy_launches, r = replay(name, B)
        assert launches == launches_from_lengths(t0, steps, B), (name, B)
        assert r.max_per_launch <= B and r.iterations == t0 + sum(t1 + t2 for t1, _, t2 in steps)
        assert r.committed_searches == 1 + sum(int(t1 > 0) + int(e) for t1, e, _ in steps) == r.env.searches
        if B < longest:
            assert busy_launches > 0 and launches > len(steps)
    # at a budget no launch's searches exceed, every launch emits and nothing is ever busy
    B = 2 * longest
    launches, busy_launches, r = replay(name, B)
    assert launches == len(steps) and busy_launches == 0 and r.max_per_launch <= 2 * longest


def test_the_issue_s_table_of_search_lengths():
    """the shapes of the GPU tests are the smallest at which the schedule can go wrong: these are the search lengths behind them"""
    t0, steps = searches_of("narrow_4x5")
    lengths = [t0] + [t for t1, e, t2 in steps for t in ((t1,) if t1 else ()) + ((t2,) if e else ())]
    assert (min(lengths), max(lengths), len(lengths)) == (18, 43, 69)
    # 2 062 iterations in all; at budget 1 a search of T iterations adds T - 1 launches, because its first iteration runs in the
    # launch that takes the action (or draws the level)
    assert sum(lengths) == 2062 and launches_from_lengths(t0, steps, 1) - len(steps) == 2062 - 69
    assert sum(int(e) for _, e, _ in searches_of("turtle_5x7_cp02")[1]) == 10  # ten episode ends


def test_a_reset_abandons_a_pending_step_without_a_trace():
    z, kw = load("narrow_8x20_p300")
    a, b = RR.SmbReadyRules(**kw), RR.SmbReadyRules(**kw)
    a.reset(10 ** 6), b.reset(10 ** 6)
    t = next(i for i, (t1, _, _) in enumerate(searches_of("narrow_8x20_p300")[1]) if t1 > 8)
    for act in z["actions"][:t]:
        a.launch(int(act), 10 ** 6), b.launch(int(act), 10 ** 6)
    status, out = a.launch(int(z["actions"][t]), 8)
    assert status == RR.BUSY and out is None and a.committed().iteration == t and np.array_equal(a.committed().grid, b.env.grid)
    a.reset(10 ** 6), b.reset(10 ** 6)  # the same next episode: the dropped step drew nothing and wrote nothing
    assert np.array_equal(a.env.grid, b.env.grid) and a.env.stats == b.env.stats and not a.busy()
    assert a.iterations == b.iterations + 8 and a.committed_searches == b.committed_searches
