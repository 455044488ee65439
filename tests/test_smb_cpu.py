"""Super Mario Bros levels, the parts that need no GPU: the plain-Python rules (tests/smb_rules.py) against the fixtures
recorded from the reference (tests/golden/smb, tools/gen_golden_smb.py), smb_spec's tables, the argument checks of the C ABI
(include/pcgrl_amd_smb.h: made before any HIP call, so they answer without a device), and what stays refused."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import smb_rules as R
from control_pcgrl_amd import _lib, problems, smb
from control_pcgrl_amd.vec_env import build_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smb")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))


def test_fixture_set_is_complete():
    assert len(FILES) == 12
    sizes = [os.path.getsize(f) for f in FILES]
    assert max(sizes) <= 100 * 1024 and sum(sizes) <= 300 * 1024


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_rules_equal_fixtures(path):
    z = np.load(path)
    power = int(z["solver_power"])
    assert list(z["stat_keys"]) == R.STAT_KEYS
    alt = dict(zip(R.STAT_KEYS, z["alt_weights"].tolist()))
    for i, m in enumerate(z["grids"]):
        stats, rec = R.get_stats(m, power)
        assert stats == z["stats"][i].tolist(), (i, stats)
        assert R.loss(stats) == z["loss"][i] and R.loss(stats, alt) == z["loss_alt"][i]
        for k, balance in ((1, 1), (2, 0)):
            p = R.run_pass(m, balance, power)
            n = int(z[f"p{k}_length"][i])
            assert p["moves"] == z[f"p{k}_moves"][i, :n].tolist() and len(p["moves"]) == n
            assert (z[f"p{k}_moves"][i, n:] == -1).all()
            assert p["iterations"] == z[f"p{k}_iterations"][i] and p["won"] == z[f"p{k}_won"][i]
            assert [p["x"], p["y"], p["air"], p["jumps"]] == z[f"p{k}_final"][i].tolist()
            locs = z[f"p{k}_jump_locs"][i]
            assert [list(l) for l in p["jump_locs"]] == locs[:len(p["jump_locs"])].tolist()
            assert (locs[len(p["jump_locs"]):] == -1).all()
        # the play-through get_stats reports is pass 1's when it wins, else pass 2's
        final = 1 if z["p1_won"][i] else 2
        assert rec["moves"] == z[f"p{final}_moves"][i, :z[f"p{final}_length"][i]].tolist()
        assert rec["it1"] == z["p1_iterations"][i] and rec["it2"] == (0 if final == 1 else z["p2_iterations"][i])


def test_spec_against_recorded_targets():
    z = np.load(FILES[0])
    for shape in ((16, 116), (8, 30)):  # frozen at the stock size whatever the map
        spec = smb.smb_spec(shape)
        assert spec.stat_keys == R.STAT_KEYS == list(z["stat_keys"]) and spec.n_tiles == 7
        for i, k in enumerate(spec.stat_keys):
            trg = spec.static_trgs[k]
            lo, hi = trg if isinstance(trg, tuple) else (trg, trg)
            assert (float(lo), float(hi)) == (z["trg_lo"][i], z["trg_hi"][i]), k
            assert float(spec.default_weights[k]) == z["weights"][i], k
            assert trg == R.STATIC_TRGS[k] and spec.default_weights[k] == R.DEFAULT_WEIGHTS[k]
        assert set(spec.cond_bounds) == set(spec.stat_keys)
    cfg = smb.smb_config((16, 116), 10000)
    assert list(cfg.trg_lo) == [0, 0, 10, 900, 0, 20, 0, 0, 348] and list(cfg.trg_hi) == [0, 0, 29, 1855, 0, 1855, 0, 0, 348]
    assert list(cfg.weight) == [2, 1, 1, 1, 4, 2, 2, 5, 1] and all(cfg.has_trg)
    with pytest.raises(ValueError):
        smb.smb_config(weights={"path-length": 1})


def test_lib_lists_the_unit_and_the_header():
    assert "smb/pcgrl_k_smb.hip" in _lib.UNITS and "smb/pcgrl_smb.h" in _lib.HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, "smb", "pcgrl_k_smb.hip")) and os.path.exists(_lib.SMB_HEADER)
    assert set(_lib.SMB_SYMBOLS) == {"pcgrl_smb_workspace_bytes", "pcgrl_smb_evaluate"}
    header = open(_lib.SMB_HEADER).read()
    for name in _lib.SMB_SYMBOLS:
        assert name + "(" in header
    assert C.sizeof(_lib.PcgrlSmbConfig) == 12 + 36 + 3 * 72


def test_abi_argument_checks_need_no_device():
    L = _lib.lib()
    assert L.pcgrl_smb_workspace_bytes(1, 16, 116, 10000) == (40001 * 12 + 15) // 16 * 16
    assert L.pcgrl_smb_workspace_bytes(4096, 16, 116, 10000) == 4096 * L.pcgrl_smb_workspace_bytes(1, 16, 116, 10000)
    for bad in ((0, 16, 116, 10000), (1, 3, 116, 10000), (1, 17, 116, 10000), (1, 16, 0, 10000), (1, 16, 129, 10000),
                (1, 16, 116, 0), (1, 16, 116, 16001)):
        assert L.pcgrl_smb_workspace_bytes(*bad) == -1, bad
    assert L.pcgrl_smb_workspace_bytes(1, 4, 1, 1) > 0 and L.pcgrl_smb_workspace_bytes(1, 16, 128, 16000) > 0

    # pointers that are never dereferenced: every call below is refused before any HIP call
    grids, ws, stats = 0x1000, 0x2000, 0x3000
    need = L.pcgrl_smb_workspace_bytes(2, 16, 116, 10000)

    def call(cfg, n=2, g=grids, w=ws, wb=need, cap=8, jcap=8, st=stats, moves=None, locs=None):
        return L.pcgrl_smb_evaluate(C.byref(cfg) if cfg is not None else None, n, g, w, wb, cap, jcap, st, None, moves, None, locs,
                                    None, None, None)

    ok = smb.smb_config((16, 116), 10000)
    EINVAL, EUNSUPPORTED = 1, 2
    assert call(None) == EINVAL
    assert call(ok, g=None) == EINVAL and call(ok, st=None) == EINVAL
    assert call(ok, n=0) == EINVAL and call(ok, n=-3) == EINVAL
    assert call(ok, w=None) == EINVAL and call(ok, wb=need - 1) == EINVAL and call(ok, w=ws + 4) == EINVAL
    assert b"workspace" in L.pcgrl_last_error()
    assert call(ok, cap=0, moves=0x4000) == EINVAL and call(ok, jcap=0, locs=0x4000) == EINVAL and call(ok, cap=-1) == EINVAL
    for shape, power in (((3, 116), 10000), ((17, 116), 10000), ((16, 129), 10000), ((16, 0), 10000), ((16, 116), 0),
                         ((16, 116), 16001)):
        assert call(smb.smb_config(shape, power)) == EUNSUPPORTED, (shape, power)
    with pytest.raises(NotImplementedError):
        smb.SmbEvaluator((3, 116), device="cuda:0")
    with pytest.raises(NotImplementedError):
        smb.SmbEvaluator((16, 116), device="cuda:0", solver_power=20000)


def test_stepping_smb_is_still_refused():
    assert "smb" not in problems.PROBLEMS
    with pytest.raises(ValueError):
        problems.problem_spec("smb", (16, 116))
    with pytest.raises(ValueError):
        build_config("smb", "narrow", (16, 116))
