"""Level measures and pairwise Hamming diversity of Super Mario Bros maps (include/pcgrl_amd_smb_measures.h) on the host: the
rules stated in numpy (tests/measures_numpy.py, T = 7) reproduce every fixture recorded from the reference
(tools/gen_golden_smb_measures.py -> tests/golden/smb_measures/) bit for bit, the fixture set holds the shapes and the cases it
has to, the ABI symbols and the unit are listed, the argument checks answer before any HIP call and the Python surface is in
place.  No GPU needed."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import measures_numpy as mn
from conftest import GOLDEN

T = 7
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "smb_measures", "*.npz")))
SHAPES = {(4, 1), (4, 2), (5, 7), (4, 65), (15, 127), (16, 116), (16, 128)}
GROUPS = {(K, G) for K in (2, 3, 5, 64, 65, 130) for G in (1, 3)}
MAX_FILE_BYTES = 38390  # the largest file under tests/golden/measures/
REF_KEYS = (("emptiness", "ref_emptiness"), ("entropy", "ref_entropy"), ("symmetry-horizontal", "ref_sym_hor"),
            ("symmetry-vertical", "ref_sym_ver"), ("symmetry", "ref_sym"), ("co-occurance", "ref_co"))
SYMBOLS = {"pcgrl_smb_measures_for_grids", "pcgrl_smb_diversity_scratch_bytes", "pcgrl_smb_diversity_for_grids",
           "pcgrl_smb_env_measures", "pcgrl_smb_env_diversity"}


def fixture_id(path):
    return os.path.basename(path)[:-4]


def fixture_shape(path):
    H, W = (int(v) for v in fixture_id(path).split("_")[1].split("x"))
    return H, W


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _cases(z):
    """(K, G, maps of the case, slice of the per-map arrays, slice of the per-group arrays) of every recorded diversity case"""
    gi = 0
    for c in range(len(z["div_K"])):
        K, G = int(z["div_K"][c]), int(z["div_G"][c])
        lo, hi = int(z["div_off"][c]), int(z["div_off"][c + 1])
        yield K, G, z["grids"][z["div_idx"][lo:hi]], slice(lo, hi), slice(gi, gi + G)
        gi += G


def test_fixture_set_is_complete():
    assert {fixture_shape(f) for f in FIXTURES} == SHAPES and len(FIXTURES) == len(SHAPES)
    assert all(os.path.getsize(f) <= MAX_FILE_BYTES for f in FIXTURES)
    for f in FIXTURES:
        z = np.load(f)  # (allow_pickle is off: arrays only)
        assert z["grids"].dtype == np.uint8 and z["grids"].shape[1:] == fixture_shape(f) and z["grids"].max() < T
        assert z["counts"].shape == (len(z["grids"]), T) and z["ref_tile_fractions"].shape == (len(z["grids"]), T)
        assert {(int(k), int(g)) for k, g in zip(z["div_K"], z["div_G"])} == GROUPS
        names = list(z["names"])
        assert {"all-0", "all-6", "symmetric", "base", "base-last-cell", "base-copy", "checker"} <= set(names)


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_numpy_rules_reproduce_the_reference_measures(path):
    z = np.load(path)
    H, W = fixture_shape(path)
    grids = z["grids"]
    cnt, mat = mn.counts(grids, T), mn.matches(grids, T)
    assert np.array_equal(cnt, z["counts"]) and np.array_equal(mat, z["match"])
    assert (cnt.sum(1) == H * W).all()
    bc = mn.bc_from_integers(cnt, mat, H, W, T)
    for key, name in REF_KEYS:
        if key == "entropy":
            continue
        assert np.array_equal(_bits(bc[key]), _bits(z[name])), key
    assert np.array_equal(_bits(mn.tile_fractions(cnt, H * W)), _bits(z["ref_tile_fractions"]))
    # entropy: bit for bit on the host that recorded the fixtures (the generator asserts it there: the same numpy log builds
    # both); numpy picks its log by the CPU's vector extensions, so on another host at most 7 terms below 0.37, each a few
    # ulps of log off, divided by ln 7: an error near 1e-15 (the bound of tests/test_measures_cpu.py)
    err = np.abs(bc["entropy"] - z["ref_entropy"]).max()
    same = np.array_equal(_bits(bc["entropy"]), _bits(z["ref_entropy"]))
    print(f"{fixture_id(path)}: entropy {'bit-equal to' if same else 'differs from'} the recorded one (max {err:.3e})")
    assert err <= 1e-13


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_numpy_rules_reproduce_the_reference_diversity(path):
    z = np.load(path)
    H, W = fixture_shape(path)
    total = 0
    for K, G, sel, maps, groups in _cases(z):
        assert len(sel) == K * G
        S, near, idx, mats = mn.diversity(sel, T, K)
        assert np.array_equal(S, z["div_sum"][groups])
        assert np.array_equal(near, z["div_nearest"][maps]) and np.array_equal(idx, z["div_nearest_idx"][maps])
        assert [mn.hamming_sum(sel[g * K:(g + 1) * K], T) for g in range(G)] == S.tolist()  # the histogram identity
        assert np.array_equal(_bits(mn.div_score(S, K, H * W)), _bits(z["div_ref_score"][groups]))
        assert np.array_equal(_bits(mn.diversity_bonus(S, K, H * W)), _bits(z["div_ref_bonus"][groups]))
        assert (mats == mats.transpose(0, 2, 1)).all() and (mats[:, np.arange(K), np.arange(K)] == 0).all()
        total += G
    assert total == len(z["div_sum"]) == len(z["div_ref_score"]) == len(z["div_ref_bonus"])


def test_fixtures_tell_the_rules_apart():
    """gen_golden_measures.check_worth's wrong rules, each failing at least one of the committed files; then the cases the 2-D
    kernel never met, visible in the recorded answers"""
    fails = dict.fromkeys(("co-wrap", "sym-divisor", "bonus-denominator", "per-bit", "tie-break", "group-leak"), 0)
    for f in FIXTURES:
        z = np.load(f)
        H, W = fixture_shape(f)
        n = H * W
        fails["co-wrap"] += not np.array_equal(mn.matches(z["grids"], T, wrap=False)[:, 2], z["match"][:, 2])
        bad = mn.bc_from_integers(z["counts"], z["match"], H, W, T, sym_divisor=max(1, W * H // 2))
        fails["sym-divisor"] += not np.array_equal(bad["symmetry-horizontal"], z["ref_sym_hor"])
        for K, G, sel, maps, groups in _cases(z):
            S = z["div_sum"][groups]
            fails["bonus-denominator"] += not np.array_equal(mn.diversity_bonus(S, K, n, denominator=K * (K - 1)),
                                                             z["div_ref_bonus"][groups])
            if K > 5 or n > 260:  # (the small cases tell these three apart; the large ones only cost time)
                continue
            for g in range(G):
                part = sel[g * K:(g + 1) * K]
                fails["per-bit"] += int(mn.pairwise(part, T, per_bit=True).sum(dtype=np.int64)) != int(S[g])
                fails["tie-break"] += not np.array_equal(mn.nearest(mn.pairwise(part, T), lowest=False)[1],
                                                         z["div_nearest_idx"][maps][g * K:(g + 1) * K])
            if G > 1:
                fails["group-leak"] += not np.array_equal(mn.nearest(mn.pairwise(sel, T))[0], z["div_nearest"][maps])
    assert all(v > 0 for v in fails.values()), fails
    # W == 1: a cell is its own horizontal neighbour, twice; no vertical-symmetry pairs
    z = np.load(os.path.join(GOLDEN, "smb_measures", "smb_4x1.npz"))
    g = z["grids"]
    assert (z["match"][:, 1] == 0).all() and (z["ref_sym_ver"] == 0.0).all()
    vert = sum((np.roll(g, s, axis=1) == g).reshape(len(g), -1).sum(1) for s in (1, -1))
    assert np.array_equal(z["match"][:, 2], 2 * 4 + vert)
    # W == 2: both horizontal rolls meet the same cell
    z = np.load(os.path.join(GOLDEN, "smb_measures", "smb_4x2.npz"))
    g = z["grids"]
    vert = sum((np.roll(g, s, axis=1) == g).reshape(len(g), -1).sum(1) for s in (1, -1))
    assert np.array_equal(z["match"][:, 2], 4 * (g[:, :, 0] == g[:, :, 1]).sum(1) + vert)
    # odd H and W: every compared cell of the symmetric map matches, and W * H / 2 = 17.5 keeps it below 1
    z = np.load(os.path.join(GOLDEN, "smb_measures", "smb_5x7.npz"))
    sym = list(z["names"]).index("symmetric")
    assert z["match"][sym, 0] == 2 * 7 and z["match"][sym, 1] == 5 * 3
    assert z["ref_sym_hor"][sym] == 14 / 17.5 < 1 and z["ref_sym_ver"][sym] == 15 / 17.5 < 1
    # W > 64: the mirror of a row's first cell is 64 cells away
    z = np.load(os.path.join(GOLDEN, "smb_measures", "smb_4x65.npz"))
    sym = list(z["names"]).index("symmetric")
    assert z["match"][sym, 1] == 4 * 32 and z["match"][sym, 0] == 2 * 65


def test_smb_measures_header_units_and_symbols():
    from control_pcgrl_amd import _lib
    _lib.build()
    assert "smb/pcgrl_k_smb_measures.hip" in _lib.UNITS and "smb/pcgrl_smb_measures.h" in _lib.HEADERS
    assert os.path.exists(_lib.SMB_MEASURES_HEADER)
    for f in ("smb/pcgrl_k_smb_measures.hip", "smb/pcgrl_smb_measures.h"):
        assert os.path.exists(os.path.join(_lib.CSRC, f))
    header = re.sub(r"/\*.*?\*/", "", open(_lib.SMB_MEASURES_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(", header))
    assert declared == SYMBOLS == set(_lib.SMB_MEASURES_SYMBOLS)
    others = [table for _, table in _lib.ABI if table is not _lib.SMB_MEASURES_SYMBOLS]
    assert len(others) == len(_lib.ABI) - 1
    assert not any(declared & set(o) for o in others)
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)  # (exported by the library)
        assert fn.argtypes == _lib.SMB_MEASURES_SYMBOLS[name][1] and fn.restype == _lib.SMB_MEASURES_SYMBOLS[name][0], name
    for name, params in re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header):
        assert len(params.split(",")) == len(_lib.SMB_MEASURES_SYMBOLS[name][1]), name
    # the kernel is plain HIP C++, and the measures header of the 2-D engine keeps its own symbol set
    src = open(os.path.join(_lib.CSRC, "smb", "pcgrl_smb_measures.h")).read()
    assert "asm" not in src.replace("namespace", "")
    assert len(_lib.MEASURES_SYMBOLS) == 6


def test_entry_points_check_their_arguments_before_any_hip_call():
    from control_pcgrl_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    p -= p % 8
    p += 8
    EINVAL, EUNSUPPORTED = 1, 2
    meas, div = L.pcgrl_smb_measures_for_grids, L.pcgrl_smb_diversity_for_grids
    # null pointers
    for args in ((16, 116, 1, None, p, p, None, None, None, None), (16, 116, 1, p, None, p, None, None, None, None),
                 (16, 116, 1, p, p, None, None, None, None, None), (16, 116, 1, p, p, p, None, p, None, None),
                 (16, 116, -1, p, p, p, None, None, None, None)):
        assert meas(*args) == EINVAL and b"pcgrl_smb_measures_for_grids:" in L.pcgrl_last_error()
    rest = (None,) * 6
    for args in ((16, 116, 8, None, 4, p, p), (16, 116, 8, p, 4, None, p), (16, 116, 8, p, 4, p, None),
                 (16, 116, 8, p, 4, p + 4, p), (16, 116, -8, p, 4, p, p)):
        assert div(*args, *rest) == EINVAL and b"pcgrl_smb_diversity_for_grids:" in L.pcgrl_last_error()
    assert L.pcgrl_smb_env_measures(None, p, p, None, None, None, None) == EINVAL
    assert b"pcgrl_smb_env_measures:" in L.pcgrl_last_error()
    assert L.pcgrl_smb_env_diversity(None, 2, p, p, None, None, None, None, None) == EINVAL
    assert b"pcgrl_smb_env_diversity:" in L.pcgrl_last_error()
    # shapes outside 4..16 x 1..128
    for h, w in ((3, 116), (16, 129), (17, 116), (16, 0)):
        assert meas(h, w, 1, p, p, p, None, None, None, None) == EUNSUPPORTED
        assert b"4..16 rows and 1..128 columns" in L.pcgrl_last_error()
        assert div(h, w, 8, p, 4, p, p, *rest) == EUNSUPPORTED
        assert L.pcgrl_smb_diversity_scratch_bytes(h, w, 8) == 0
    # group 1, and group 3 of 8 maps
    for group in (1, 3, 0, -2):
        assert div(16, 116, 8, p, group, p, p, *rest) == EINVAL
        assert b"group must be at least 2 and divide the number of maps" in L.pcgrl_last_error()
    # no maps: a no-op
    assert meas(16, 116, 0, None, None, None, None, None, None, None) == 0
    assert div(16, 116, 0, None, 4, None, None, None, None, None, None, None) == 0
    assert L.pcgrl_smb_diversity_scratch_bytes(16, 116, 0) == 0
    assert L.pcgrl_smb_diversity_scratch_bytes(16, 116, 4096) == 4096 * (3 * 29 + 1) * 8
    assert L.pcgrl_smb_diversity_scratch_bytes(4, 1, 3) == 3 * (3 + 1) * 8
    assert L.pcgrl_smb_diversity_scratch_bytes(16, 128, 1) == (3 * 32 + 1) * 8


def test_python_surface_is_in_place():
    import inspect

    from control_pcgrl_amd import SmbEvaluator, SmbGymEnv, SmbReadyVecEnv, SmbVecEnv
    assert list(inspect.signature(SmbEvaluator.measures).parameters) == ["self", "grids", "entropy"]
    assert list(inspect.signature(SmbEvaluator.diversity).parameters) == ["self", "grids", "group", "pairwise"]
    for cls in (SmbVecEnv, SmbReadyVecEnv):
        assert list(inspect.signature(cls.measures).parameters) == ["self", "entropy"]
        assert list(inspect.signature(cls.measures_for_grids).parameters) == ["self", "grids", "entropy"]
        assert list(inspect.signature(cls.diversity).parameters) == ["self", "group", "pairwise"]
        assert list(inspect.signature(cls.diversity_for_grids).parameters) == ["self", "grids", "group", "pairwise"]
    assert SmbReadyVecEnv.measures is SmbVecEnv.measures and SmbReadyVecEnv.diversity is SmbVecEnv.diversity
    assert isinstance(SmbGymEnv.measures, property)
    for fn, default in ((SmbEvaluator.measures, True), (SmbVecEnv.measures, True), (SmbVecEnv.measures_for_grids, True)):
        assert inspect.signature(fn).parameters["entropy"].default is default
    for fn in (SmbEvaluator.diversity, SmbVecEnv.diversity, SmbVecEnv.diversity_for_grids):
        sig = inspect.signature(fn).parameters
        assert sig["group"].default is None and sig["pairwise"].default is False
