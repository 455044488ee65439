"""The twin engines of tests/test_gpu_step16.py and tests/test_gpu_step_masks.py: the same config, seeds and actions on
step16_kernel (the default) and on step_kernel (PCGRL_STEP16=0, the development switch read once at pcgrl_create), and how
the two and the CPU oracle are compared after a call."""
import os

import numpy as np
import torch

REW_TOL = 1e-6
SHAPE = (16, 16)
EMPTY = {"narrow": 0, "turtle": 4}  # the action that makes the cell under `pos` passable; + 1: solid


def _pair(rep, n, seeds, auto_reset, **kw):
    """(step16 engine, step_kernel engine): the switch is read once, at pcgrl_create"""
    from control_pcgrl_amd import VecPcgrlEnv
    assert "PCGRL_STEP16" not in os.environ
    new = VecPcgrlEnv("binary", rep, SHAPE, n, seeds=seeds, auto_reset=auto_reset, **kw)
    os.environ["PCGRL_STEP16"] = "0"
    try:
        old = VecPcgrlEnv("binary", rep, SHAPE, n, seeds=seeds, auto_reset=auto_reset, **kw)
    finally:
        del os.environ["PCGRL_STEP16"]
    return new, old


def _same(a, b, what):
    assert torch.equal(a, b), what


def _image(env):
    """pcgrl_export_state into a zero-filled buffer (the image's sections are padded: the padding is not written)"""
    import ctypes as C
    from control_pcgrl_amd import _lib
    blob = torch.zeros(int(env._L.pcgrl_state_bytes(env._h)), dtype=torch.uint8, device=env.device)
    _lib.check(env._L.pcgrl_export_state(env._h, blob.data_ptr(), C.byref(C.c_int32(0)), env._stream()), "pcgrl_export_state")
    return blob


def _compare(new, old, out_new, out_old, t):
    for k, name in enumerate(("obs", "reward", "done")):
        _same(out_new[k], out_old[k], f"{name} @ {t}")
    _same(out_new[4]["stats"], out_old[4]["stats"], f"stats @ {t}")
    _same(_image(new), _image(old), f"state image @ {t}")


def _step_all(new, old, orc, a, t, auto_reset):
    dev_a = torch.as_tensor(a, dtype=torch.int32).to(new.device)
    on, oo = new.step(dev_a), old.step(dev_a)
    _compare(new, old, on, oo, t)
    _, orew, odone, ostats = orc.step(np.asarray(a, np.int32), auto_reset=auto_reset, want_obs=False)
    assert np.array_equal(on[4]["stats"].cpu().numpy(), ostats), f"stats vs oracle @ {t}"
    assert np.max(np.abs(on[1].cpu().numpy().astype(np.float64) - orew)) <= REW_TOL, f"reward vs oracle @ {t}"
    assert np.array_equal(on[2].cpu().numpy(), odone), f"done vs oracle @ {t}"
    return odone
