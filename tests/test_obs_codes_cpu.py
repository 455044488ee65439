"""The tile-code observation form (include/pcgrl_amd_codes.h) on the host: ABI symbols, argument checks, shapes, and
codes_to_onehot against numpy.  No GPU needed."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_codes_header_symbols_exported_and_bound():
    from control_pcgrl_amd import _lib
    _lib.build()
    header = open(os.path.join(ROOT, "include", "pcgrl_amd_codes.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z_]+)\s*\(", header))
    assert declared >= {"pcgrl_codes_shape", "pcgrl_codes_bytes", "pcgrl_observe_codes", "pcgrl_onehot_to_codes"}
    assert set(_lib.CODES_SYMBOLS) == declared
    assert not declared & set(_lib.SYMBOLS)  # (pcgrl_amd.h's table stays what that header declares)
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)
        assert fn.argtypes == _lib.CODES_SYMBOLS[name][1], name


def test_codes_entry_points_refuse_null_handles_and_pointers():
    from control_pcgrl_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint8 * 64)()
    shape, nd = (C.c_int32 * 4)(), C.c_int32()
    assert L.pcgrl_codes_shape(None, C.byref(shape), C.byref(nd)) == 1
    assert L.pcgrl_codes_shape(None, None, None) == 1
    assert L.pcgrl_codes_bytes(None) == -1
    assert L.pcgrl_observe_codes(None, C.addressof(buf), None) == 1
    assert L.pcgrl_observe_codes(None, None, None) == 1
    assert L.pcgrl_onehot_to_codes(None, C.addressof(buf), 1, C.addressof(buf), None) == 1
    assert L.pcgrl_onehot_to_codes(None, None, 1, None, None) == 1
    assert L.pcgrl_step_ready_codes(None, C.addressof(buf), 1, C.addressof(buf), C.addressof(buf), None, None, None,
                                    C.addressof(buf), None) == 1
    assert L.pcgrl_step_ready_codes(None, None, 1, None, None, None, None, None, None, None) == 1
    assert b"bad arguments" in L.pcgrl_last_error()


def _env(problem, rep, shape, static=False):
    return SimpleNamespace(problem=problem, representation=rep, map_shape=shape,
                           obs_shape=(1, 1, 2 if static else 1))


@pytest.mark.parametrize("problem,rep,shape,static,c", [
    ("binary", "narrow", (16, 16), False, 3), ("zelda", "turtle", (16, 16), False, 9), ("zelda", "narrow", (16, 16), True, 9),
    ("sokoban", "wide", (16, 16), False, 5), ("minecraft_3D_maze", "narrow", (7, 7, 7), False, 4)])
def test_codes_to_onehot_matches_numpy(problem, rep, shape, static, c):
    from control_pcgrl_amd import codes_to_onehot
    rng = np.random.default_rng(3)
    lead = (5,) + tuple(2 * s for s in shape) if rep != "wide" else (5,) + shape
    codes = rng.integers(0, c, size=lead + (1,), dtype=np.uint8)
    want = np.eye(c, dtype=np.uint8)[codes[..., 0]]
    if static:
        st = rng.integers(0, 2, size=lead + (1,), dtype=np.uint8)
        codes = np.concatenate((codes, st), axis=-1)
        want = np.concatenate((want, st), axis=-1)
    got = codes_to_onehot(torch.as_tensor(codes), _env(problem, rep, shape, static))
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert np.array_equal(got.numpy(), want)


@pytest.mark.parametrize("problem,rep,shape,kw,onehot,codes", [
    ("binary", "narrow", (16, 16), {}, (32, 32, 3), (32, 32, 1)),
    ("zelda", "turtle", (16, 16), {}, (32, 32, 9), (32, 32, 1)),
    ("zelda", "narrow", (16, 16), {"static_prob": 0.1, "n_static_walls": 2}, (32, 32, 10), (32, 32, 2)),
    ("binary", "narrow", (16, 16), {"obs_window": (15, 9)}, (15, 9, 3), (15, 9, 1)),
    ("binary", "narrow", (16, 16), {"act_window": (3, 3)}, (32, 32, 3), (32, 32, 1)),
    ("sokoban", "wide", (16, 16), {}, (16, 16, 5), (16, 16, 1)),
    ("minecraft_3D_maze", "narrow", (7, 7, 7), {}, (14, 14, 14, 4), (14, 14, 14, 1)),
])
def test_codes_shape_table(problem, rep, shape, kw, onehot, codes):
    from control_pcgrl_amd.vec_env import build_config, obs_shape_for
    cfg, spec, ow = build_config(problem, rep, shape, obs_window=kw.get("obs_window"), act_window=kw.get("act_window"),
                                 static_prob=kw.get("static_prob"), n_static_walls=kw.get("n_static_walls"))
    assert obs_shape_for(cfg, spec, ow, "onehot") == onehot
    assert obs_shape_for(cfg, spec, ow, "codes") == codes


def test_unknown_obs_format_raises():
    from control_pcgrl_amd import SubBatchedVecEnv, VecPcgrlEnv, make_vec_env
    from control_pcgrl_amd.vec_env import build_config, obs_shape_for
    with pytest.raises(ValueError, match="obs_format"):
        VecPcgrlEnv("binary", "narrow", (16, 16), 4, obs_format="bogus")
    with pytest.raises(ValueError, match="obs_format"):
        SubBatchedVecEnv("binary", "narrow", (16, 16), 4, 2, obs_format="bogus")
    cfg = {"task": {"problem": "binary", "map_shape": (16, 16)}, "representation": "narrow", "obs_format": "bogus"}
    with pytest.raises(ValueError, match="obs_format"):
        make_vec_env(cfg, 4)
    c, spec, ow = build_config("binary", "narrow", (16, 16))
    with pytest.raises(ValueError, match="obs_format"):
        obs_shape_for(c, spec, ow, "one-hot")
