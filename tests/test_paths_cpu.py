"""Solution paths (include/pcgrl_amd_paths.h) on the host: the rules stated in numpy (tests/paths_numpy.py) replay every
fixture recorded from the reference (tools/gen_golden_paths.py -> tests/golden/paths/), the ABI symbols, the argument checks.
No GPU needed."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import paths_numpy as pn
from conftest import GOLDEN, ROOT

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "paths", "*.npz")))
SHAPES = {"8x8", "5x40", "16x16", "12x40", "24x20", "20x40", "40x24", "40x48", "1x1", "1x5", "5x1", "7x11", "32x32", "64x64"}


def test_fixture_set_is_complete():
    names = {os.path.basename(f)[:-4] for f in FIXTURES}
    assert names == {f"{p}_{s}" for p in ("binary", "zelda") for s in SHAPES}
    assert sum(os.path.getsize(f) for f in FIXTURES) < 300 * 1024


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
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


def test_fixtures_hold_the_longest_path_a_map_can_have():
    z = np.load(os.path.join(GOLDEN, "paths", "binary_64x64.npz"))
    assert np.diff(z["offsets"]).max() == 2080 and z["L"].max() == 2079  # the serpentine


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
