"""Solution paths (include/pcgrl_amd_paths.h) on the host: the rules stated in numpy (tests/paths_numpy.py) replay every
fixture recorded from the reference (tools/gen_golden_paths.py -> tests/golden/paths/ and its structured/ sub-folder), what the
structured set has to contain to be worth replaying, the ABI symbols, the argument checks.  No GPU needed."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import paths_numpy as pn
from conftest import GOLDEN, ROOT

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "paths", "*.npz")))
STRUCTURED = sorted(glob.glob(os.path.join(GOLDEN, "paths", "structured", "*.npz")))
STRUCTURED_SHAPES = {"8x8", "5x7", "16x16", "20x24", "40x16", "12x40", "40x48", "64x64"}
SHAPES = {"8x8", "5x40", "16x16", "12x40", "24x20", "20x40", "40x24", "40x48", "1x1", "1x5", "5x1", "7x11", "32x32", "64x64"}


def test_fixture_set_is_complete():
    names = {os.path.basename(f)[:-4] for f in FIXTURES}
    assert names == {f"{p}_{s}" for p in ("binary", "zelda") for s in SHAPES}
    assert sum(os.path.getsize(f) for f in FIXTURES) < 300 * 1024


def test_structured_set_is_complete():
    names = {os.path.basename(f)[:-4] for f in STRUCTURED}
    assert names == {f"{p}_{s}" for p in ("binary", "zelda") for s in STRUCTURED_SHAPES}
    assert all(os.path.getsize(f) <= 16 * 1024 for f in STRUCTURED)
    assert sum(os.path.getsize(f) for f in STRUCTURED) <= 100 * 1024


@pytest.mark.parametrize("path", FIXTURES + STRUCTURED, ids=[os.path.basename(f)[:-4] for f in FIXTURES]
                         + ["structured_" + os.path.basename(f)[:-4] for f in STRUCTURED])
def test_numpy_rules_replay_the_reference(path):
    z = np.load(path)
    problem = os.path.basename(path).split("_")[0]
    grids, cells, off = z["grids"], z["cells"], z["offsets"]
    assert grids.dtype == np.uint8 and cells.dtype == np.int16 and off.shape == (len(grids) + 1,) and off[-1] == len(cells)
    for i, g in enumerate(grids):
        want = [tuple(c) for c in cells[off[i]:off[i + 1]].tolist()]
        if problem == "binary":
            got, length = pn.binary_path(g)
            assert length == z["L"][i], i
            assert len(got) == (length + 1 if length else 0), i
        else:
            got = pn.zelda_path(g)
        assert got == want, (i, g.tolist())


def test_fixtures_hold_the_serpentine_and_the_longest_known_path():
    z = np.load(os.path.join(GOLDEN, "paths", "binary_64x64.npz"))
    assert np.diff(z["offsets"]).max() == 2080 and z["L"].max() == 2079  # the serpentine
    # ... which is not the longest path a 64 x 64 map can have: the one-cell-wide spiral has 2 111 cells (the bound is n_cells)
    z = np.load(os.path.join(GOLDEN, "paths", "structured", "binary_64x64.npz"))
    spiral = list(z["names"]).index("spiral")
    assert np.diff(z["offsets"])[spiral] == 2111 and z["L"][spiral] == 2110 and z["L"].max() == 2110
    assert np.diff(z["offsets"])[list(z["names"]).index("serpentine")] == 2080


@pytest.mark.parametrize("shape", sorted(STRUCTURED_SHAPES))
def test_structured_files_hold_long_repeated_and_half_paths(shape):
    """what the structured set is for: per shape a binary and a zelda path of at least n_cells / 2 cells, a zelda path that
    walks a cell twice (both halves pass the player's cell: more cells than the overlay has), a path of one half only (the
    other half's target is cut off), and the key and the door at every distance 1..7 from the player the width allows"""
    h, w = (int(v) for v in shape.split("x"))
    zb = np.load(os.path.join(GOLDEN, "paths", "structured", f"binary_{shape}.npz"))
    zz = np.load(os.path.join(GOLDEN, "paths", "structured", f"zelda_{shape}.npz"))
    for z in (zb, zz):
        assert z["names"].shape == (len(z["grids"]),) and z["grids"].shape[1:] == (h, w)
        assert 2 * np.diff(z["offsets"]).max() >= h * w
    assert {"spiral", "comb", "checkerboard", "equal-rooms", "open-frame", "staircase", "two-cells-last-row",
            "one-cell-last-corner", "serpentine", "serpentine-transposed"} == set(zb["names"])
    assert zb["L"][list(zb["names"]).index("checkerboard")] == 0 and zb["L"][list(zb["names"]).index("one-cell-last-corner")] == 0
    assert zb["L"][list(zb["names"]).index("two-cells-last-row")] == 1
    off, cells, grids = zz["offsets"], zz["cells"], zz["grids"]
    repeated = half_only = 0
    for i, g in enumerate(grids):
        path = [tuple(c) for c in cells[off[i]:off[i + 1]].tolist()]
        repeated += len(path) > len(set(path))
        if path:
            (p,), (k,), (d,) = (np.argwhere(g == t) for t in (pn.PLAYER, pn.KEY, pn.DOOR))
            a = pn.trace(pn.bfs((g != pn.SOLID) & (g != pn.DOOR), tuple(p)), tuple(k))
            b = pn.trace(pn.bfs(g != pn.SOLID, tuple(k)), tuple(d))
            half_only += (len(a) == 0) != (len(b) == 0)
    assert repeated >= 1 and half_only >= 1
    names = set(zz["names"])
    for d in range(1, 8):
        if d + 1 < w:
            assert {f"{ground}-{first}-first-d{d}" for ground in ("open", "row0") for first in ("key", "door")} <= names
    for i, name in enumerate(zz["names"]):  # the names say where the tiles are
        if "-first-d" in name:
            d = int(name[-1])
            pair = (pn.KEY, pn.DOOR) if "-key-first" in name else (pn.DOOR, pn.KEY)
            assert grids[i][0, 0] == pn.PLAYER and tuple(grids[i][0, d:d + 2]) == pair
            assert (grids[i][1:] == (pn.SOLID if name.startswith("row0") else pn.EMPTY)).all()


def test_paths_header_symbols_exported_and_bound():
    from control_pcgrl_amd import _lib
    _lib.build()
    header = open(os.path.join(ROOT, "include", "pcgrl_amd_paths.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z_]+)\s*\(", header))
    assert declared == {"pcgrl_path_capacity", "pcgrl_paths", "pcgrl_paths_for_grids"}
    assert set(_lib.PATHS_SYMBOLS) == declared
    assert not declared & (set(_lib.SYMBOLS) | set(_lib.CODES_SYMBOLS) | set(_lib.ASYNC3D_SYMBOLS))
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)
        assert fn.argtypes == _lib.PATHS_SYMBOLS[name][1] and fn.restype == _lib.PATHS_SYMBOLS[name][0], name
    # the declarations' parameter counts are the bound ones
    for name, params in re.findall(r"\b(pcgrl_[a-z_]+)\s*\(([^)]*)\)\s*;", header):
        assert len(params.split(",")) == len(_lib.PATHS_SYMBOLS[name][1]), name


def test_path_entry_points_refuse_bad_arguments_by_name():
    from control_pcgrl_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    assert L.pcgrl_path_capacity(None) == -1
    for args in ((None, 4, p, p, None, None), (None, 4, None, None, None, None), (None, 0, p, p, p, None)):
        assert L.pcgrl_paths(*args) == 1
        assert b"pcgrl_paths:" in L.pcgrl_last_error()
    for args in ((None, 1, p, 4, p, p, None, None), (None, 1, None, 4, None, None, None, None), (None, 1, p, 0, p, p, None, None),
                 (None, -1, p, 4, p, p, None, None)):
        assert L.pcgrl_paths_for_grids(*args) == 1
        assert b"pcgrl_paths_for_grids:" in L.pcgrl_last_error()
