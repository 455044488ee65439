"""Checkpoint and restore of Super Mario Bros environments, the part that needs no GPU: the ABI's header, symbol table and unit,
its refusals before any HIP call, the Python methods, and the rules of tests/smb_state_rules.py against themselves -- a run that
is exported, imported into another (dirty) rules env and continued equals the uninterrupted run, without a budget and at budgets
1 and 8, where the image is taken with searches parked."""
import inspect
import os
import re
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smb_env_rules as E  # noqa: E402
import smb_ready_rules as RR  # noqa: E402
import smb_rules as R  # noqa: E402
import smb_state_rules as SR  # noqa: E402

from control_pcgrl_amd import _lib, smb_env, smb_ready  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smb_env")
EINVAL = 1
FIXTURES = ["narrow_4x5", "turtle_5x7_cp02"]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes()) & 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------- the ABI

def test_lib_lists_the_unit_the_header_and_the_symbols():
    assert "smb/pcgrl_k_smb_state.hip" in _lib.UNITS and "smb/pcgrl_smb_state.h" in _lib.HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, "smb", "pcgrl_k_smb_state.hip"))
    assert os.path.exists(os.path.join(_lib.CSRC, "smb", "pcgrl_smb_state.h")) and os.path.exists(_lib.SMB_STATE_HEADER)
    header = open(_lib.SMB_STATE_HEADER).read()
    declared = set(re.findall(r"\b(pcgrl_smb_state_\w+)\(", header))
    assert set(_lib.SMB_STATE_SYMBOLS) == declared and len(declared) == 6
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(pcgrl_\w+)\(", code)) == declared  # nothing else is declared here
    others = [table for _, table in _lib.ABI if table is not _lib.SMB_STATE_SYMBOLS]
    assert len(others) == len(_lib.ABI) - 1
    for table in others:
        assert not declared & set(table)
    for path in (_lib.HEADER, _lib.SMB_HEADER, _lib.SMB_ENV_HEADER, _lib.SMB_READY_HEADER):  # and no other header declares them
        assert not re.findall(r"\bpcgrl_smb_state_\w+\(", open(path).read()), path
    L = _lib.lib()
    for name, (res, args) in _lib.SMB_STATE_SYMBOLS.items():
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype == res, name
        params = re.search(name + r"\(([^;]*)\);", header, re.S).group(1)
        assert len(params.split(",")) == len(args), name


def test_every_entry_point_refuses_a_null_handle_without_a_device():
    L = _lib.lib()
    calls = [("pcgrl_smb_state_export", (None, 0x1000, None)), ("pcgrl_smb_state_import", (None, None, None, 0x1000, None)),
             ("pcgrl_smb_state_set", (None, None, 0x1000, 0x1000, 0x1000, 0x1000, None)),
             ("pcgrl_smb_state_get_rng", (None, 0x1000, None)), ("pcgrl_smb_state_set_rng", (None, None, 0x1000, None))]
    for name, args in calls:
        assert getattr(L, name)(*args) == EINVAL, name
        assert name.encode() in L.pcgrl_last_error() and b"null handle" in L.pcgrl_last_error(), name
        assert getattr(L, name)(*([None] * len(args))) == EINVAL, name
    assert L.pcgrl_smb_state_bytes(None) == -1 and b"pcgrl_smb_state_bytes: null handle" in L.pcgrl_last_error()


def test_the_python_methods_and_their_signatures():
    from control_pcgrl_amd import SmbReadyVecEnv, SmbVecEnv
    want = {"export_state": ["self", "out"], "get_rng_state": ["self"], "set_rng_state": ["self", "rng", "mask"],
            "set_state": ["self", "grids", "pos", "counters", "ep_return", "mask"], "state_dict": ["self"],
            "load_state_dict": ["self", "sd", "mask", "index"]}
    for name, params in want.items():
        fn = getattr(SmbVecEnv, name)
        sig = inspect.signature(fn)
        assert list(sig.parameters) == params, name
        assert all(p.default is None for k, p in sig.parameters.items() if k in ("out", "mask", "index")), name
        assert getattr(SmbReadyVecEnv, name) is fn, name  # inherited, not overridden
    assert isinstance(SmbVecEnv.state_bytes, property) and SmbReadyVecEnv.state_bytes is SmbVecEnv.state_bytes
    assert SmbReadyVecEnv is smb_ready.SmbReadyVecEnv and SmbVecEnv is smb_env.SmbVecEnv
    assert not hasattr(smb_env.SmbGymEnv, "state_dict")  # pickling the gym env is out of scope


# ----------------------------------------------------------------------------------------- the rules against themselves

def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cp = float(z["change_percentage"])
    kw = dict(representation=str(z["representation"]), shape=tuple(int(s) for s in z["map_shape"]),
              obs_window=tuple(int(s) for s in z["obs_window"]), weights={k: float(w) for k, w in zip(R.STAT_KEYS, z["weights"])},
              change_percentage=None if cp < 0 else cp, solver_power=int(z["solver_power"]))
    return z, kw


def moments(z):
    """the three kinds of t (steps taken before the export): mid-episode, the step before an episode end, the step after one"""
    ends = np.nonzero(z["done"])[0]
    assert len(ends) and ends[0] >= 4 and ends[0] + 2 < len(z["actions"])
    d = int(ends[0])
    return [d // 2, d, d + 1]


def row(out):
    return (out["reward"], bool(out["done"]), tuple(out["stats"]), tuple(out["pos"]), out["iteration"], out["changes"],
            crc(out["obs"]))


def dirty(rules, z, steps=5):
    """a rules env of another seed that has been stepped: its map, counters and streams are not the exporter's"""
    rules.reset()
    for a in z["actions"][:steps]:
        rules.step(int(a), auto_reset=True)
    return rules


@pytest.mark.parametrize("name", FIXTURES)
def test_a_restored_run_equals_the_uninterrupted_one(name):
    z, kw = load(name)
    seed, actions = int(z["seed"]), z["actions"]

    def step(r, t):
        obs, reward, done, info = r.step(int(actions[t]), auto_reset=True)
        stats = info["final_stats"] if "final_stats" in info else info["stats"]
        return (reward, bool(done), tuple(stats), tuple(r.pos), crc(obs))

    whole = E.SmbEnvRules(seed=seed, **kw)
    whole.reset()
    want = [step(whole, t) for t in range(len(actions))]
    for t, w in enumerate(want):  # the uninterrupted run is the fixture
        assert w == (float(z["reward"][t]), bool(z["done"][t]), tuple(z["stats"][t].tolist()), tuple(z["pos"][t].tolist()),
                     int(z["obs_crc"][t])), t
    for t0 in moments(z):
        a = E.SmbEnvRules(seed=seed, **kw)
        a.reset()
        for t in range(t0):
            step(a, t)
        image = SR.export(a)
        b = dirty(E.SmbEnvRules(seed=seed + 1, **kw), z)
        SR.import_(b, image)
        assert [step(b, t) for t in range(t0, len(actions))] == want[t0:], (name, t0)  # the next episodes' maps included
        assert b.searches == whole.searches and b.ep_return == whole.ep_return
        assert step(a, t0) == want[t0]
        assert image["env"].iteration == (0 if z["done"][t0 - 1] else t0)  # (the first episode: t0 steps into it, or a fresh one)
        # the image is a copy: the exporter went on, the image did not
        c = E.SmbEnvRules(seed=seed + 2, **kw)
        SR.import_(c, image)
        assert step(c, t0) == want[t0]


def run_ready(r, actions, budget, t=0, until_progress=None, until_mode=None, limit=200000):
    """launches at `budget`, feeding actions[t], actions[t + 1], ... when the env takes one -> (t, emitted rows, launches);
    stops when t reaches until_progress, or after the first launch that leaves the env in until_mode"""
    rows, launches = [], 0
    while t < len(actions) or r.busy():
        if until_progress is not None and t >= until_progress:
            break
        taking = not r.busy()
        status, out = r.launch(int(actions[t]) if taking and t < len(actions) else -7, budget)
        launches += 1
        assert launches <= limit
        t += int(taking)
        if out is not None:
            rows.append(row(out))
        assert bool(status & RR.BUSY) == r.busy()
        if until_mode is not None and r.mode == until_mode:
            break
    return t, rows, launches


@pytest.mark.parametrize("budget", [1, 8])
@pytest.mark.parametrize("name", FIXTURES)
def test_a_restored_run_equals_the_uninterrupted_one_under_a_budget(name, budget):
    z, kw = load(name)
    seed, actions = int(z["seed"]), z["actions"]
    whole = SR.SmbReadyStateRules(seed=seed, **kw)
    whole.reset(budget)
    _, want, whole_launches = run_ready(whole, actions, budget)
    assert len(want) == len(actions)
    for t, w in enumerate(want):  # the uninterrupted run emits the fixture
        assert w[:3] == (float(z["reward"][t]), bool(z["done"][t]), tuple(z["stats"][t].tolist())) and w[6] == int(z["obs_crc"][t])
    # an image at each of the three moments, whatever the env is doing then, and one in each mode
    stops = [dict(until_progress=t0) for t0 in moments(z)] + [dict(until_mode=m) for m in (SR.PENDING_STEP, SR.PENDING_STATS)]
    seen_modes = set()
    for stop in stops:
        a = SR.SmbReadyStateRules(seed=seed, **kw)
        a.reset(budget)
        t, head, la = run_ready(a, actions, budget, **stop)
        if "until_mode" in stop:
            assert a.mode == stop["until_mode"], (name, budget, stop)
        seen_modes.add(a.mode)
        image = SR.export(a)
        assert image["iterations"] == a.iterations - SR.in_flight(a) and 0 <= SR.in_flight(a) < RR.search_length(a.env) + 1
        b = SR.SmbReadyStateRules(seed=seed + 1, **kw)
        b.reset(budget)
        run_ready(b, actions, budget, until_progress=5)  # dirty, and possibly with a search parked
        SR.import_(b, image)
        assert b.mode == a.mode and b.busy() == a.busy() and b.committed_searches == a.committed_searches
        assert np.array_equal(b.committed().grid, a.committed().grid) and b.committed_stats() == a.committed_stats()
        _, tail, lb = run_ready(b, actions, budget, t=t)
        assert head + tail == want, (name, budget, stop)
        # every counter but the launch count: the restarted search runs its first iterations a second time
        assert b.iterations == whole.iterations and b.committed_searches == whole.committed_searches == b.env.searches
        assert la + lb >= whole_launches and la + lb - whole_launches <= -(-SR.in_flight(a) // budget)
        # the same image into an env without a budget: only an idle row
        c = dirty(E.SmbEnvRules(seed=seed + 2, **kw), z)
        if a.mode != SR.IDLE:
            with pytest.raises(NotImplementedError):
                SR.import_(c, image)
        else:
            SR.import_(c, image)
            if t < len(actions):
                obs, reward, done, info = c.step(int(actions[t]), auto_reset=True)
                assert (reward, bool(done), crc(obs)) == (want[t][0], want[t][1], want[t][6])
    assert seen_modes == {SR.IDLE, SR.PENDING_STEP, SR.PENDING_STATS}


def test_an_image_without_a_budget_imports_into_a_budgeted_env():
    z, kw = load("narrow_4x5")
    seed, actions = int(z["seed"]), z["actions"]
    a = E.SmbEnvRules(seed=seed, **kw)
    a.reset()
    t0 = moments(z)[1]
    for t in range(t0):
        a.step(int(actions[t]), auto_reset=True)
    b = SR.SmbReadyStateRules(seed=seed + 1, **kw)
    b.reset(1)
    run_ready(b, actions, 1, until_mode=SR.PENDING_STEP)
    SR.import_(b, SR.export(a))
    assert b.mode == SR.IDLE and not b.busy() and b.committed_searches == a.searches
    _, tail, _ = run_ready(b, actions, 3, t=t0)
    for k, w in enumerate(tail):
        t = t0 + k
        assert w[:3] == (float(z["reward"][t]), bool(z["done"][t]), tuple(z["stats"][t].tolist())) and w[6] == int(z["obs_crc"][t])
    assert len(tail) == len(actions) - t0
