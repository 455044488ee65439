"""Level measures and pairwise Hamming diversity of Lode Runner maps (include/pcgrl_amd_loderunner_measures.h) on the host: the
rules stated in numpy (tests/measures_numpy.py, T = 8) reproduce every fixture recorded from the reference
(tools/gen_golden_loderunner_measures.py -> tests/golden/loderunner_measures/) bit for bit, the fixture set holds the shapes and
the cases it has to, the ABI symbols and the unit are listed, the argument checks answer before any HIP call and the Python
surface is in place.  No GPU needed."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import measures_numpy as mn
from conftest import GOLDEN

T = 8
DIR = os.path.join(GOLDEN, "loderunner_measures")
FIXTURES = sorted(glob.glob(os.path.join(DIR, "*.npz")))
SHAPES = {(1, 1), (2, 1), (1, 2), (1, 32), (16, 1), (5, 7), (8, 12), (15, 31), (16, 32)}
GROUPS = {(K, G) for K in (2, 3, 5, 64, 65, 130) for G in (1, 3)}
MAX_FILE_BYTES = 38390  # the largest file under tests/golden/measures/
REF_KEYS = (("emptiness", "ref_emptiness"), ("entropy", "ref_entropy"), ("symmetry-horizontal", "ref_sym_hor"),
            ("symmetry-vertical", "ref_sym_ver"), ("symmetry", "ref_sym"), ("co-occurance", "ref_co"))
SYMBOLS = {"pcgrl_loderunner_measures_for_grids", "pcgrl_loderunner_diversity_scratch_bytes",
           "pcgrl_loderunner_diversity_for_grids"}


def fixture_id(path):
    return os.path.basename(path)[:-4]


def fixture_shape(path):
    H, W = (int(v) for v in fixture_id(path).split("_")[1].split("x"))
    return H, W


def _load(H, W):
    return np.load(os.path.join(DIR, f"lr_{H}x{W}.npz"))


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
        assert {"all-0", "all-7", "symmetric", "base", "base-last-cell", "base-copy", "checker"} <= set(names)


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_numpy_rules_reproduce_the_reference_measures(path):
    z = np.load(path)
    H, W = fixture_shape(path)
    grids = z["grids"]
    cnt, mat = mn.counts(grids, T), mn.matches(grids, T)
    assert np.array_equal(cnt, z["counts"]) and np.array_equal(mat, z["match"])
    assert (cnt.sum(1) == H * W).all()  # with T = 8 every id is a counted tile
    bc = mn.bc_from_integers(cnt, mat, H, W, T)
    for key, name in REF_KEYS:
        if key == "entropy":
            continue
        assert np.array_equal(_bits(bc[key]), _bits(z[name])), key
    assert np.array_equal(_bits(mn.tile_fractions(cnt, H * W)), _bits(z["ref_tile_fractions"]))
    # entropy: bit for bit on the host that recorded the fixtures (the generator asserts it there: the same numpy log builds
    # both); numpy picks its log by the CPU's vector extensions, so on another host at most 8 terms below 0.37, each a few
    # ulps of log off, divided by ln 8: an error near 1e-15 (the bound of tests/test_measures_cpu.py)
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
    """gen_golden_measures.check_worth's wrong rules, each failing at least one of the committed files; then the cases this
    shape range brings, visible in the recorded answers"""
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


def test_one_row_and_one_column():
    # H == 1: no horizontal-symmetry pairs; a cell is its own vertical neighbour, twice
    for H, W in ((1, 32), (1, 2), (1, 1)):
        z = _load(H, W)
        g = z["grids"]
        assert (z["match"][:, 0] == 0).all() and (z["ref_sym_hor"] == 0.0).all()
        hor = sum((np.roll(g, s, axis=2) == g).reshape(len(g), -1).sum(1) for s in (1, -1))
        assert np.array_equal(z["match"][:, 2], 2 * W + hor)
    # W == 1: the same along the other axis
    for H, W in ((16, 1), (2, 1)):
        z = _load(H, W)
        g = z["grids"]
        assert (z["match"][:, 1] == 0).all() and (z["ref_sym_ver"] == 0.0).all()
        vert = sum((np.roll(g, s, axis=1) == g).reshape(len(g), -1).sum(1) for s in (1, -1))
        assert np.array_equal(z["match"][:, 2], 2 * H + vert)
    # W == 2 (H == 2): both rolls along that axis meet the same cell
    z = _load(1, 2)
    g = z["grids"]
    assert np.array_equal(z["match"][:, 2], 2 * 2 + 4 * (g[:, 0, 0] == g[:, 0, 1]))
    z = _load(2, 1)
    g = z["grids"]
    assert np.array_equal(z["match"][:, 2], 2 * 2 + 4 * (g[:, 0, 0] == g[:, 1, 0]))


def test_a_single_cell():
    """1 x 1: no symmetry pairs over the divisor 0.5; every co-occurance comparison is the cell against itself"""
    z = _load(1, 1)
    assert (z["match"] == [0, 0, 4]).all()
    assert (z["ref_sym_hor"] == 0.0).all() and (z["ref_sym_ver"] == 0.0).all() and (z["ref_sym"] == 0.0).all()
    assert (z["ref_co"] == 1.0).all()
    assert np.array_equal(z["ref_emptiness"], (z["grids"][:, 0, 0] == 0).astype(np.float64))
    assert (z["ref_entropy"] == 0.0).all() and (z["counts"].sum(1) == 1).all()
    bc = mn.bc_from_integers(z["counts"], z["match"], 1, 1, T)
    assert (bc["symmetry-horizontal"] == 0 / 0.5).all() and (bc["co-occurance"] == 1.0).all()


def test_odd_sizes_and_full_chunks():
    # odd H and W: every compared cell of the symmetric map matches, and W * H / 2 = 17.5 keeps it below 1
    z = _load(5, 7)
    sym = list(z["names"]).index("symmetric")
    assert z["match"][sym, 0] == 2 * 7 and z["match"][sym, 1] == 5 * 3
    assert z["ref_sym_hor"][sym] == 14 / 17.5 < 1 and z["ref_sym_ver"][sym] == 15 / 17.5 < 1
    z = _load(15, 31)
    sym = list(z["names"]).index("symmetric")
    assert z["match"][sym, 0] == 7 * 31 and z["match"][sym, 1] == 15 * 15 and z["ref_sym_hor"][sym] == 217 / 232.5
    # 16 x 32: eight full chunks -- the last cell is bit 63 of word 7, and the file tells a map from its last-cell variant
    z = _load(16, 32)
    assert z["grids"].shape[1] * z["grids"].shape[2] == 512 == 8 * 64
    names = list(z["names"])
    a, b = z["grids"][names.index("base")], z["grids"][names.index("base-last-cell")]
    diff = np.flatnonzero((a != b).reshape(-1))
    assert diff.tolist() == [511]
    assert not np.array_equal(z["counts"][names.index("base")], z["counts"][names.index("base-last-cell")])
    sym = names.index("symmetric")
    assert z["match"][sym, 0] == 8 * 32 and z["match"][sym, 1] == 16 * 16 and z["ref_sym"][sym] == 1.0
    # the divisors are the map's own H * W, not the 12 x 8 the problem's targets are frozen at
    zero = names.index("all-0")
    assert z["ref_emptiness"][zero] == 1.0 and z["counts"][zero, 0] == 512 and z["ref_co"][zero] == 1.0


def test_loderunner_measures_header_units_and_symbols():
    from control_pcgrl_amd import _lib
    _lib.build()
    units = ("loderunner/pcgrl_k_loderunner_measures.hip",)
    headers = ("loderunner/pcgrl_loderunner_measures.h", "measures/pcgrl_measures_wave.h")
    assert all(u in _lib.UNITS for u in units) and all(h in _lib.HEADERS for h in headers)
    assert os.path.exists(_lib.LODERUNNER_MEASURES_HEADER)
    for f in units + headers:
        assert os.path.exists(os.path.join(_lib.CSRC, f))
    header = re.sub(r"/\*.*?\*/", "", open(_lib.LODERUNNER_MEASURES_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(", header))
    assert declared == SYMBOLS == set(_lib.LODERUNNER_MEASURES_SYMBOLS)
    others = [table for _, table in _lib.ABI if table is not _lib.LODERUNNER_MEASURES_SYMBOLS]
    assert len(others) == len(_lib.ABI) - 1
    assert not any(declared & set(o) for o in others)
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)  # (exported by the library)
        want = _lib.LODERUNNER_MEASURES_SYMBOLS[name]
        assert fn.argtypes == want[1] and fn.restype == want[0], name
    for name, params in re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header):
        assert len(params.split(",")) == len(_lib.LODERUNNER_MEASURES_SYMBOLS[name][1]), name
    # the kernel and the shared wave body are plain HIP C++; the wave body is written once and the kernel instantiates it
    for f in headers:
        src = open(os.path.join(_lib.CSRC, f)).read()
        assert "asm" not in src.replace("namespace", ""), f
    kernel = open(os.path.join(_lib.CSRC, headers[0])).read()
    assert "meas_wave_map<LR_MEAS_TILES, LR_MEAS_PLANES, LR_MEAS_MAX_CELLS>" in kernel and "__ballot" not in kernel
    # what the existing tables pin stays
    assert set(_lib.LODERUNNER_SYMBOLS) == {"pcgrl_loderunner_workspace_bytes", "pcgrl_loderunner_evaluate"}
    assert len(_lib.MEASURES_SYMBOLS) == 6 and len(_lib.SMB_MEASURES_SYMBOLS) == 5
    assert b"0.7.0" in L.pcgrl_version()


def test_entry_points_check_their_arguments_before_any_hip_call():
    from control_pcgrl_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    p -= p % 8
    p += 8
    EINVAL, EUNSUPPORTED = 1, 2
    meas, div = L.pcgrl_loderunner_measures_for_grids, L.pcgrl_loderunner_diversity_for_grids
    scratch = L.pcgrl_loderunner_diversity_scratch_bytes
    # null pointers, entropy without its table, n < 0
    for args in ((8, 12, 1, None, p, p, None, None, None, None), (8, 12, 1, p, None, p, None, None, None, None),
                 (8, 12, 1, p, p, None, None, None, None, None), (8, 12, 1, p, p, p, None, p, None, None),
                 (8, 12, -1, p, p, p, None, None, None, None)):
        assert meas(*args) == EINVAL and b"pcgrl_loderunner_measures_for_grids:" in L.pcgrl_last_error()
    rest = (None,) * 6
    # null grids, scratch, sum; a scratch that is not 8-byte aligned; n < 0
    for args in ((8, 12, 8, None, 4, p, p), (8, 12, 8, p, 4, None, p), (8, 12, 8, p, 4, p, None), (8, 12, 8, p, 4, p + 4, p),
                 (8, 12, -8, p, 4, p, p)):
        assert div(*args, *rest) == EINVAL and b"pcgrl_loderunner_diversity_for_grids:" in L.pcgrl_last_error()
    # shapes outside 1..16 x 1..32
    for h, w in ((0, 12), (17, 12), (8, 0), (8, 33)):
        assert meas(h, w, 1, p, p, p, None, None, None, None) == EUNSUPPORTED
        assert b"1..16 rows and 1..32 columns" in L.pcgrl_last_error()
        assert div(h, w, 8, p, 4, p, p, *rest) == EUNSUPPORTED
        assert b"1..16 rows and 1..32 columns" in L.pcgrl_last_error()
        assert scratch(h, w, 8) == 0
    # group 1, and group 3 of 8 maps
    for group in (1, 3, 0, -2):
        assert div(8, 12, 8, p, group, p, p, *rest) == EINVAL
        assert b"group must be at least 2 and divide the number of maps" in L.pcgrl_last_error()
    # no maps: a no-op
    assert meas(8, 12, 0, None, None, None, None, None, None, None) == 0
    assert div(8, 12, 0, None, 4, None, None, None, None, None, None, None) == 0
    assert scratch(8, 12, 0) == 0 and scratch(8, 12, -3) == 0
    # 8 * (3 * ceil(h * w / 64) + 1) per map
    assert scratch(1, 1, 3) == 3 * (3 * 1 + 1) * 8
    assert scratch(8, 12, 4096) == 4096 * (3 * 2 + 1) * 8
    assert scratch(16, 32, 1) == (3 * 8 + 1) * 8
    assert scratch(8, 8, 1) == (3 * 1 + 1) * 8 and scratch(5, 13, 1) == (3 * 2 + 1) * 8  # 64 cells: one word; 65: two


def test_python_surface_is_in_place():
    import inspect

    import control_pcgrl_amd
    from control_pcgrl_amd import LODERUNNER_BC_NAMES, LodeRunnerEvaluator, loderunner
    assert list(inspect.signature(LodeRunnerEvaluator.measures).parameters) == ["self", "grids", "entropy"]
    assert list(inspect.signature(LodeRunnerEvaluator.diversity).parameters) == ["self", "grids", "group", "pairwise"]
    assert list(inspect.signature(LodeRunnerEvaluator.behaviour).parameters) == ["self", "grids", "names"]
    assert inspect.signature(LodeRunnerEvaluator.measures).parameters["entropy"].default is True
    sig = inspect.signature(LodeRunnerEvaluator.diversity).parameters
    assert sig["group"].default is None and sig["pairwise"].default is False
    # evaluate() and check_errors() keep their signatures
    assert list(inspect.signature(LodeRunnerEvaluator.evaluate).parameters) == ["self", "grids", "gold_cap"]
    assert inspect.signature(LodeRunnerEvaluator.evaluate).parameters["gold_cap"].default == 32
    assert list(inspect.signature(LodeRunnerEvaluator.check_errors).parameters) == ["self"]
    # get_bc's names: the five statistics first (it looks in stats first), the six measures, "NONE"
    assert LODERUNNER_BC_NAMES is loderunner.LODERUNNER_BC_NAMES is control_pcgrl_amd.LODERUNNER_BC_NAMES
    assert tuple(LODERUNNER_BC_NAMES) == ("player", "enemies", "gold", "win", "path-length", "emptiness", "entropy", "symmetry",
                                          "symmetry-horizontal", "symmetry-vertical", "co-occurance", "NONE")
    assert tuple(LODERUNNER_BC_NAMES[:5]) == tuple(loderunner.LODERUNNER_STAT_KEYS)
    assert tuple(LODERUNNER_BC_NAMES[5:11]) == tuple(mn.BC_NAMES) == tuple(loderunner.LODERUNNER_MEASURE_NAMES)
    assert len(loderunner.LODERUNNER_TILES) == T
    doc = loderunner.__doc__
    assert "stepping Lode Runner environments is not built" in doc and "measures" in doc
