"""Open-loop rollouts of Super Mario Bros environments, the part that needs no GPU: the ABI's header, symbol table and unit, its
refusals before any HIP call, the host form of the device-drawn actions, and the Python layer's refusals."""
import inspect
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

from control_pcgrl_amd import _lib, smb_env, smb_ready

EINVAL = 1
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------- the ABI

def test_lib_lists_the_unit_the_header_and_the_symbols():
    assert "smb/pcgrl_k_smb_rollout.hip" in _lib.UNITS and "smb/pcgrl_smb_rollout.h" in _lib.HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, "smb", "pcgrl_k_smb_rollout.hip"))
    assert os.path.exists(os.path.join(_lib.CSRC, "smb", "pcgrl_smb_rollout.h")) and os.path.exists(_lib.SMB_ROLLOUT_HEADER)
    header = open(_lib.SMB_ROLLOUT_HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_\w+)\(", code))
    assert set(_lib.SMB_ROLLOUT_SYMBOLS) == declared and len(declared) == 3
    others = [table for _, table in _lib.ABI if table is not _lib.SMB_ROLLOUT_SYMBOLS]
    assert len(others) == len(_lib.ABI) - 1
    for table in others:
        assert not declared & set(table)
    for path in (_lib.HEADER, _lib.SMB_HEADER, _lib.SMB_ENV_HEADER, _lib.SMB_READY_HEADER, _lib.SMB_STATE_HEADER):
        text = open(path).read()  # no other header declares them
        assert not any(re.search(r"\b" + name + r"\(", text) for name in declared), path
    L = _lib.lib()
    for name, (res, args) in _lib.SMB_ROLLOUT_SYMBOLS.items():
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype == res, name
        params = re.search(name + r"\(([^;]*)\);", code, re.S).group(1)
        assert len(params.split(",")) == len(args), name
    assert b"0.7.0" in L.pcgrl_version()  # the state image is unchanged, and so is the version


def rollout_args(h=None, actions=None, seed=0, n_steps=4, auto_reset=1, obs=None, obs_mode=0):
    return (h, actions, seed, n_steps, auto_reset, obs, obs_mode) + (None,) * 10


def test_a_null_handle_is_refused_without_a_device():
    L = _lib.lib()
    assert L.pcgrl_smb_env_num_actions(None) == -1
    assert L.pcgrl_smb_env_rollout(*rollout_args()) == EINVAL
    assert b"pcgrl_smb_env_rollout" in L.pcgrl_last_error() and b"null handle" in L.pcgrl_last_error()
    assert L.pcgrl_smb_env_rollout(*rollout_args(actions=0x1000, obs=0x1000, obs_mode=2)) == EINVAL
    assert L.pcgrl_smb_env_rollout(None, 0x1000, 0, 4, 1, 0x1000, 1, *([0x1000] * 9), None) == EINVAL
    assert L.pcgrl_smb_env_sample_actions(None, 0x1000, 0, None) == EINVAL
    assert b"pcgrl_smb_env_sample_actions" in L.pcgrl_last_error()
    assert L.pcgrl_smb_env_sample_actions(None, None, 0, None) == EINVAL


# ------------------------------------------------------------------------------------------------- the drawn actions

def mix64(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def one_action(seed, c, i, n):
    """the header's formula in Python integers"""
    r = mix64(mix64((seed + c * 0x9e3779b97f4a7c15) & M64) ^ ((i * 0xd1b54a32d192ed03 + 0x8cb92ba72f3d8dd7) & M64))
    return (r * n) >> 64


@pytest.mark.parametrize("seed,first,n_act", [(0, 0, 7), (3, 5, 11), (M64, 2 ** 40 + 1, 7), (2 ** 63 + 12345, M64 - 1, 11)])
def test_sampled_actions_is_the_headers_function(seed, first, n_act):
    a = smb_env.sampled_actions(seed, first, 6, 70, n_act)
    assert a.shape == (6, 70) and a.dtype == np.int32
    want = [[one_action(seed, (first + k) & M64, i, n_act) for i in range(70)] for k in range(6)]
    assert a.tolist() == want


def test_sampled_actions_properties():
    a = smb_env.sampled_actions(9, 4, 50, 257, 7)
    assert np.array_equal(a, smb_env.sampled_actions(9, 4, 50, 257, 7))  # deterministic
    assert a.min() == 0 and a.max() == 6  # inside [0, num_actions), and over 12 850 draws both ends occur
    b = smb_env.sampled_actions(9, 4, 50, 257, 11)
    assert b.min() == 0 and b.max() == 10
    for k in (0, 1, 17, 49):  # row k of a call starting at draw c is row 0 of a call starting at draw c + k
        assert np.array_equal(a[k], smb_env.sampled_actions(9, 4 + k, 1, 257, 7)[0]), k
    assert not np.array_equal(a, smb_env.sampled_actions(10, 4, 50, 257, 7))  # the seed matters
    assert not np.array_equal(a[0], a[1]) and len(set(a[:, 0].tolist())) > 1 and len(set(a[0].tolist())) > 1
    assert np.array_equal(a[:, :64], smb_env.sampled_actions(9, 4, 50, 64, 7))  # an env's draws do not depend on the batch size
    counts = np.bincount(a.ravel(), minlength=7) / a.size
    assert np.abs(counts - 1 / 7).max() < 0.02  # 12 850 draws: a standard deviation of 0.003 per cell


# ------------------------------------------------------------------------------------------------------ the Python layer

def test_the_python_methods_and_their_signatures():
    from control_pcgrl_amd import SmbReadyVecEnv, SmbVecEnv
    sig = inspect.signature(SmbVecEnv.rollout)
    assert list(sig.parameters) == ["self", "actions", "n_steps", "want_obs", "seed"]
    assert [p.default for p in sig.parameters.values()][1:] == [None, None, "last", 0]
    sig = inspect.signature(SmbVecEnv.sample_actions)
    assert list(sig.parameters) == ["self", "seed", "out"] and sig.parameters["out"].default is None
    assert SmbReadyVecEnv.sample_actions is SmbVecEnv.sample_actions
    assert list(inspect.signature(smb_env.sampled_actions).parameters) == ["seed", "first_draw", "n_steps", "num_envs",
                                                                           "num_actions"]
    assert not hasattr(smb_env.SmbGymEnv, "rollout")  # the gym env steps one action at a time


def test_the_ready_class_refuses_by_name_while_a_budget_is_set():
    with pytest.raises(NotImplementedError, match="SmbReadyVecEnv.rollout: a solver budget is set.*busy.*step_ready"):
        smb_ready.SmbReadyVecEnv.rollout(NS(solver_budget=8), None, n_steps=4)
    seen = []

    class Base(smb_env.SmbVecEnv):
        def __init__(self):
            pass

    class Ready(smb_ready.SmbReadyVecEnv):
        solver_budget = 0

        def __init__(self):
            pass

    # without a budget it is the base class's: the argument checks below are smb_env.SmbVecEnv.rollout's
    assert smb_ready.SmbReadyVecEnv.__mro__[1] is smb_env.SmbVecEnv
    for env in (Base(), Ready()):
        env.num_envs = 3
        with pytest.raises(ValueError, match="want_obs"):
            env.rollout(n_steps=2, want_obs="first")
        with pytest.raises(ValueError, match="n_steps"):
            env.rollout()
        with pytest.raises(ValueError, match=r"\[K, 3\]"):
            env.rollout(np.zeros((2, 4), np.int32))
        seen.append(type(env).__name__)
    assert seen == ["Base", "Ready"]
