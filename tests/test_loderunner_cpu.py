"""Lode Runner levels, the parts that need no GPU: the plain-Python rules (tests/loderunner_rules.py) against the fixtures
recorded from the reference with its clock stopped (tests/golden/loderunner, tools/gen_golden_loderunner.py), loderunner_spec's
tables, the argument checks of the C ABI (include/pcgrl_amd_loderunner.h: made before any HIP call, so they answer without a
device), the restated loss on hand-computed cases, and what stays refused."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import loderunner_rules as R
from control_pcgrl_amd import _lib, loderunner, problems
from control_pcgrl_amd.vec_env import build_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loderunner")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))
SHAPES = {(8, 12), (1, 1), (2, 1), (1, 5), (4, 4), (5, 7), (16, 32), (3, 9)}


def test_fixture_set_is_complete():
    assert len(FILES) == 11
    assert {tuple(np.load(f)["grids"].shape[1:]) for f in FILES} == SHAPES
    sizes = [os.path.getsize(f) for f in FILES]
    assert max(sizes) <= 100 * 1024 and sum(sizes) <= 300 * 1024


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_rules_equal_fixtures(path):
    z = np.load(path)
    assert list(z["stat_keys"]) == R.STAT_KEYS
    cap = z["gold_state"].shape[1]
    for i, m in enumerate(z["grids"]):
        stats, play, gs, gd = R.outputs(m, cap)
        assert np.asarray(stats).tobytes() == z["stats"][i].tobytes(), (i, stats)
        assert play == [int(z["stats"][i, 0] == 1), *z["landing"][i].tolist(), int(z["collected"][i])], (i, play)
        assert gs == z["gold_state"][i].tolist() and gd == z["gold_dist"][i].tolist(), i
        assert int((z["gold_state"][i] >= 0).sum()) == stats[2]


def test_spec_tables():
    for shape in ((8, 12), (16, 32)):  # frozen at the stock size whatever the map
        spec = loderunner.loderunner_spec(shape)
        assert spec.name == "loderunner" and spec.stat_keys == R.STAT_KEYS and spec.tile_types == R.TILES and spec.n_tiles == 8
        assert spec.static_trgs == R.STATIC_TRGS and spec.static_trgs["path-length"] == 103.0
        assert spec.cond_bounds == R.COND_BOUNDS and spec.default_weights == R.DEFAULT_WEIGHTS == spec.problem_weights
    cfg = loderunner.loderunner_config((8, 12))
    assert (cfg.h, cfg.w) == (8, 12) and all(cfg.has_trg)
    assert list(cfg.trg_lo) == [1, 2, 1, 1, 103] and list(cfg.trg_hi) == [1, 2, 9, 1, 103]  # (1, 10) excludes 10
    assert list(cfg.weight) == [1, 0, 0, 1, 0]
    assert R.target_interval((1, 10)) == problems.target_interval((1, 10)) == (1.0, 9.0)
    with pytest.raises(ValueError):
        loderunner.loderunner_config(weights={"sol-length": 1})


def test_loss_of_the_rules_on_hand_computed_cases():
    w = {"player": 1, "enemies": 2, "gold": 4, "win": 8, "path-length": 0.5}
    # on every target: no loss
    assert R.loss([1, 2, 9, 1, 103], w) == 0.0 and R.loss([1, 2, 1, 1.0, 103], w) == 0.0
    # 3 players (2 off), 0 enemies (2 off), 10 golds (1 above the interval 1..9), win 0.25 (0.75 off), path-length 20 (83 off)
    assert R.loss([3, 0, 10, 0.25, 20], w) == -(2 * 1 + 2 * 2 + 1 * 4 + 0.75 * 8 + 83 * 0.5) == -57.5
    # a fractional win with the default weights: 1 / 3 is not dyadic, the term is one rounded subtraction and multiplication
    assert R.loss([1, 5, 3, 1 / 3, 40]) == -(1.0 - 1 / 3) * 1.0
    # no gold: win = -1 is 2 off; no player: 1 off
    assert R.loss([1, 0, 0, -1, 0]) == -2.0 and R.loss([0, 0, 4, 0, 0]) == -2.0
    assert R.loss([2, 2, 0, 0, 0], {"player": 3, "gold": 5}) == -(1 * 3 + 1 * 5)


def test_lib_lists_the_unit_and_the_header():
    assert "loderunner/pcgrl_k_loderunner.hip" in _lib.UNITS and "loderunner/pcgrl_loderunner.h" in _lib.HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, "loderunner", "pcgrl_k_loderunner.hip")) and os.path.exists(_lib.LODERUNNER_HEADER)
    assert set(_lib.LODERUNNER_SYMBOLS) == {"pcgrl_loderunner_workspace_bytes", "pcgrl_loderunner_evaluate"}
    others = [table for _, table in _lib.ABI if table is not _lib.LODERUNNER_SYMBOLS]
    assert len(others) == len(_lib.ABI) - 1
    assert not any(set(_lib.LODERUNNER_SYMBOLS) & set(o) for o in others)
    header = open(_lib.LODERUNNER_HEADER).read()
    L = _lib.lib()
    for name, (res, args) in _lib.LODERUNNER_SYMBOLS.items():
        fn = getattr(L, name)  # exported and bound
        assert fn.argtypes == args and fn.restype == res, name
        params = header.split(name + "(")[1].split(")")[0]
        assert len(params.split(",")) == len(args), name
    assert C.sizeof(_lib.PcgrlLoderunnerConfig) == 8 + 20 + 4 + 3 * 40


def test_abi_argument_checks_need_no_device():
    L = _lib.lib()

    def per_block(h, w):
        return (4 * h * w + 1 + h + w + h * w + 1 + h * w) * 64 * 4

    assert L.pcgrl_loderunner_workspace_bytes(1, 8, 12) == per_block(8, 12)
    assert L.pcgrl_loderunner_workspace_bytes(1000, 8, 12) == 1000 * per_block(8, 12)
    # one slot per block of the launch; the blocks stop at what fits 640 MiB, at least 256 and at most 4096, whatever n
    assert L.pcgrl_loderunner_workspace_bytes(100000, 8, 12) == L.pcgrl_loderunner_workspace_bytes(4096, 8, 12) == 4096 * per_block(8, 12)
    assert L.pcgrl_loderunner_workspace_bytes(4096, 16, 32) == ((640 << 20) // per_block(16, 32)) * per_block(16, 32) == 839 * per_block(16, 32)
    assert L.pcgrl_loderunner_workspace_bytes(838, 16, 32) == 838 * per_block(16, 32)
    assert L.pcgrl_loderunner_workspace_bytes(1, 1, 1) == per_block(1, 1) and L.pcgrl_loderunner_workspace_bytes(1, 16, 32) == per_block(16, 32)
    for bad in ((0, 8, 12), (-1, 8, 12), (1, 0, 12), (1, 17, 12), (1, 8, 0), (1, 8, 33), (1, -1, 12)):
        assert L.pcgrl_loderunner_workspace_bytes(*bad) == -1, bad

    # pointers that are never dereferenced: every call below is refused before any HIP call
    grids, ws, stats = 0x1000, 0x2000, 0x3000
    need = L.pcgrl_loderunner_workspace_bytes(2, 8, 12)

    def call(cfg, n=2, g=grids, w=ws, wb=need, cap=8, st=stats):
        return L.pcgrl_loderunner_evaluate(C.byref(cfg) if cfg is not None else None, n, g, w, wb, cap, st, None, None, None, None,
                                           None, None)

    ok = loderunner.loderunner_config((8, 12))
    EINVAL, EUNSUPPORTED = 1, 2
    assert call(None) == EINVAL
    assert call(ok, g=None) == EINVAL and call(ok, st=None) == EINVAL
    assert call(ok, n=0) == EINVAL and call(ok, n=-3) == EINVAL
    assert call(ok, cap=-1) == EINVAL
    assert call(ok, w=None) == EINVAL and call(ok, wb=need - 1) == EINVAL and call(ok, w=ws + 2) == EINVAL
    assert b"workspace" in L.pcgrl_last_error()
    for shape in ((0, 12), (17, 12), (8, 0), (8, 33)):
        assert call(loderunner.loderunner_config(shape)) == EUNSUPPORTED, shape
    assert b"1..16 rows and 1..32 columns" in L.pcgrl_last_error()
    for shape in ((0, 12), (17, 12), (8, 33)):
        with pytest.raises(NotImplementedError):
            loderunner.LodeRunnerEvaluator(shape, device="cuda:0")
    with pytest.raises(ValueError):
        loderunner.LodeRunnerEvaluator((8, 12), device="cpu")  # no CPU fallback
    with pytest.raises(ValueError):
        loderunner.LodeRunnerEvaluator((8, 12, 2))


def test_loderunner_stays_outside_the_engine():
    import control_pcgrl_amd
    assert control_pcgrl_amd.LodeRunnerEvaluator is loderunner.LodeRunnerEvaluator
    assert control_pcgrl_amd.loderunner_spec is loderunner.loderunner_spec
    assert "loderunner" not in problems.PROBLEMS and "loderunner_ctrl" not in problems.PROBLEMS
    with pytest.raises(ValueError):
        problems.problem_spec("loderunner", (8, 12))
    with pytest.raises(ValueError):
        build_config("loderunner", "narrow", (8, 12))
    assert control_pcgrl_amd.__version__ == "0.7.0" and b"0.7.0" in _lib.lib().pcgrl_version()
