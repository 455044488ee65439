"""Level measures and pairwise Hamming diversity (include/pcgrl_amd_measures.h) on the host: the rules stated in numpy
(tests/measures_numpy.py) reproduce every fixture recorded from the reference (tools/gen_golden_measures.py ->
tests/golden/measures/), the fixture set holds what it has to, the ABI symbols and units are listed, the argument checks and
the refusals are in place.  No GPU needed."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import measures_numpy as mn
from conftest import GOLDEN, ROOT

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "measures", "*.npz")))
SHAPES = {"1x1", "1x5", "5x1", "2x2", "2x7", "7x11", "8x8", "16x16", "12x40", "64x64"}
GROUPS = {(K, G) for K in (2, 3, 5, 64, 65, 130) for G in (1, 3)}


def fixture_id(path):
    return os.path.basename(path)[:-4]


def fixture_meta(path):
    problem, shape = fixture_id(path).split("_")
    H, W = (int(v) for v in shape.split("x"))
    return problem, mn.N_TILES[problem], H, W


def test_fixture_set_is_complete():
    # (sokoban's largest map is 62 x 62: the engine's solver level is the map plus its border, at most 64 x 64)
    want = {f"{p}_{s}" for p in mn.N_TILES for s in SHAPES} - {"sokoban_64x64"} | {"sokoban_62x62"}
    assert {fixture_id(f) for f in FIXTURES} == want
    assert sum(os.path.getsize(f) for f in FIXTURES) < 600 * 1024
    assert all(os.path.getsize(f) < 64 * 1024 for f in FIXTURES)


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_numpy_rules_reproduce_the_reference_measures(path):
    z = np.load(path)
    problem, T, H, W = fixture_meta(path)
    grids = z["grids"]
    assert grids.dtype == np.uint8 and grids.shape[1:] == (H, W) and grids.max() < T
    cnt, mat = mn.counts(grids, T), mn.matches(grids, T)
    assert np.array_equal(cnt, z["counts"]) and np.array_equal(mat, z["match"])
    assert (cnt.sum(1) == H * W).all()
    bc = mn.bc_from_integers(cnt, mat, H, W, T)
    # bit for bit -- entropy too whenever this host's numpy log equals the recording host's; 1e-13 otherwise (at most 8 terms
    # below 0.37, each a few ulps of log off, divided by at least ln 2: an error near 1e-15)
    for key, name in (("emptiness", "ref_emptiness"), ("symmetry-horizontal", "ref_sym_hor"),
                      ("symmetry-vertical", "ref_sym_ver"), ("symmetry", "ref_sym"), ("co-occurance", "ref_co")):
        assert np.array_equal(bc[key], z[name]), key
    assert np.array_equal(mn.tile_fractions(cnt, H * W), z["ref_tile_fractions"])
    assert np.abs(bc["entropy"] - z["ref_entropy"]).max() <= 1e-13


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_numpy_rules_reproduce_the_reference_diversity(path):
    z = np.load(path)
    problem, T, H, W = fixture_meta(path)
    assert {(int(k), int(g)) for k, g in zip(z["div_K"], z["div_G"])} == GROUPS
    gi = 0
    for c in range(len(z["div_K"])):
        K, G = int(z["div_K"][c]), int(z["div_G"][c])
        lo, hi = int(z["div_off"][c]), int(z["div_off"][c + 1])
        assert hi - lo == K * G
        sel = z["grids"][z["div_idx"][lo:hi]]
        S, near, idx, mats = mn.diversity(sel, T, K)
        assert np.array_equal(S, z["div_sum"][gi:gi + G])
        assert np.array_equal(near, z["div_nearest"][lo:hi]) and np.array_equal(idx, z["div_nearest_idx"][lo:hi])
        assert [mn.hamming_sum(sel[g * K:(g + 1) * K], T) for g in range(G)] == S.tolist()  # the histogram identity
        assert np.array_equal(mn.div_score(S, K, H * W), z["div_ref_score"][gi:gi + G])
        assert np.array_equal(mn.diversity_bonus(S, K, H * W), z["div_ref_bonus"][gi:gi + G])
        assert (mats == mats.transpose(0, 2, 1)).all() and (mats[:, np.arange(K), np.arange(K)] == 0).all()
        gi += G
    assert gi == len(z["div_sum"]) == len(z["div_ref_score"])


def test_fixtures_tell_the_rules_apart():
    """the quirks of the contract, each visible in the recorded answers"""
    z = np.load(os.path.join(GOLDEN, "measures", "zelda_7x11.npz"))
    names = list(z["names"])
    sym = names.index("symmetric")
    assert z["match"][sym, 0] == 3 * 11 and z["match"][sym, 1] == 7 * 5  # every compared cell matches ...
    assert z["ref_sym_hor"][sym] == 33 / 38.5 < 1 and z["ref_sym_ver"][sym] == 35 / 38.5 < 1  # ... and W * H / 2 = 38.5
    a0, a7 = names.index("all-0"), names.index("all-7")
    assert mn.pairwise(z["grids"][[a0, a7]], 8)[0, 1] == 77  # three differing bits, one per cell
    assert z["ref_co"][a0] == 1.0 and z["ref_entropy"][a0] == 0.0 and z["ref_emptiness"][a0] == 1.0
    base, last, copy = (names.index(n) for n in ("base", "base-last-cell", "base-copy"))
    d = mn.pairwise(z["grids"][[base, last, copy]], 8)
    assert d.tolist() == [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
    assert (z["grids"][base] != z["grids"][last]).nonzero()[0].tolist() == [6]  # the very last cell
    # the wrapped rolls: one row is its own vertical neighbour, two rows meet the same cell twice
    z15 = np.load(os.path.join(GOLDEN, "measures", "binary_1x5.npz"))
    assert (z15["match"][:, 2] >= 2 * 5).all()
    z27 = np.load(os.path.join(GOLDEN, "measures", "binary_2x7.npz"))
    g = z27["grids"]
    assert np.array_equal(z27["match"][:, 2] - mn.matches(g, 2, wrap=False)[:, 2],
                          2 * (g[:, 0] == g[:, 1]).sum(1) + 2 * (g[:, :, 0] == g[:, :, -1]).sum(1))
    # the bonus denominator is K * K - 1
    K = int(z["div_K"][0])
    assert z["div_ref_bonus"][0] == 10 * (int(z["div_sum"][0]) / (K * K - 1)) / 77


def test_measures_header_units_and_symbols():
    from control_pcgrl_amd import _lib
    _lib.build()
    assert "measures/pcgrl_k_measures.hip" in _lib.UNITS and "measures/pcgrl_measures.h" in _lib.HEADERS
    assert os.path.exists(_lib.MEASURES_HEADER)
    for f in ("measures/pcgrl_k_measures.hip", "measures/pcgrl_measures.h"):
        assert os.path.exists(os.path.join(_lib.CSRC, f))
    header = open(_lib.MEASURES_HEADER).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z_]+)\s*\(", header))
    assert declared == {"pcgrl_measures_tiles", "pcgrl_measures", "pcgrl_measures_for_grids", "pcgrl_diversity_scratch_bytes",
                        "pcgrl_diversity", "pcgrl_diversity_for_grids"}
    assert set(_lib.MEASURES_SYMBOLS) == declared
    assert not declared & (set(_lib.SYMBOLS) | set(_lib.CODES_SYMBOLS) | set(_lib.PATHS_SYMBOLS) | set(_lib.SOLUTIONS_SYMBOLS))
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)
        assert fn.argtypes == _lib.MEASURES_SYMBOLS[name][1] and fn.restype == _lib.MEASURES_SYMBOLS[name][0], name
    for name, params in re.findall(r"\b(pcgrl_[a-z_]+)\s*\(([^)]*)\)\s*;", header):
        assert len(params.split(",")) == len(_lib.MEASURES_SYMBOLS[name][1]), name
    # no inline assembly in the kernels
    src = open(os.path.join(_lib.CSRC, "measures", "pcgrl_measures.h")).read()
    assert "asm" not in src.replace("namespace", "")


def test_measure_entry_points_refuse_bad_arguments_by_name():
    from control_pcgrl_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    assert L.pcgrl_measures_tiles(None) == -1
    assert L.pcgrl_diversity_scratch_bytes(None, 4) == 0
    assert L.pcgrl_measures(None, p, p, None, None, None, None) == 1 and b"pcgrl_measures:" in L.pcgrl_last_error()
    assert L.pcgrl_measures_for_grids(None, 1, p, p, p, None, None, None, None) == 1
    assert b"pcgrl_measures_for_grids:" in L.pcgrl_last_error()
    assert L.pcgrl_diversity(None, 2, p, p, None, None, None, None, None) == 1 and b"pcgrl_diversity:" in L.pcgrl_last_error()
    assert L.pcgrl_diversity_for_grids(None, 2, p, 2, p, p, None, None, None, None, None) == 1
    assert b"pcgrl_diversity_for_grids:" in L.pcgrl_last_error()


def test_refusal_messages_are_present():
    """the reasons, where a user meets them: the 3-D maze (C), sub-batches and multi-agent batches (Python)"""
    from control_pcgrl_amd import _lib
    engine = open(os.path.join(_lib.CSRC, "pcgrl_engine.hip")).read()
    assert "get_counts reads an attribute the 3-D maze does not have" in engine and "get_co looks at two" in engine
    assert "group must be at least 2 and divide the number of maps" in engine
    import inspect

    from control_pcgrl_amd import multiagent, vec_env
    src = inspect.getsource(vec_env.SubBatchedVecEnv.diversity)
    assert "NotImplementedError" in src and "straddle" in src and "diversity_for_grids" in src
    for fn in (multiagent.MultiAgentVecEnv.measures, multiagent.MultiAgentVecEnv.diversity):
        assert "NotImplementedError" in inspect.getsource(fn)
    assert "single-agent" in multiagent.MultiAgentVecEnv._NO_MEASURES
    assert all(hasattr(vec_env.VecPcgrlEnv, m) for m in ("measures", "measures_for_grids", "diversity", "diversity_for_grids"))
    assert hasattr(vec_env.SubBatchedVecEnv, "measures")
