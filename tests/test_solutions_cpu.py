"""Sokoban solutions (include/pcgrl_amd_solutions.h) on the host: the ABI symbols, the argument checks, the fixtures recorded
from the reference (tools/gen_golden_solutions.py -> tests/golden/solutions/): what the set has to contain to be worth
replaying, every solution replayed to a win, and the plain-Python rules (tests/sokoban_rules.py) against every recorded
answer, move for move.  No GPU needed."""
import ctypes as C
import glob
import json
import os
import re

import numpy as np
import pytest

import sokoban_rules as sr
from conftest import GOLDEN, ROOT

SOL = os.path.join(GOLDEN, "solutions")
ROOMS = sorted(glob.glob(os.path.join(SOL, "rooms_*.npz")))
ROOM_SHAPES = {"8x8", "16x16", "20x20", "30x30", "40x24", "20x40", "48x33", "62x62"}
# solved levels of the committed solver fixtures, per source array (35 in all: 26 at 16 x 16, 1 at 8 x 8, 3 at 20 x 20, 1 at
# 20 x 40, 3 at 48 x 33, 1 at 62 x 62)
FIXTURE_SOLVED = {"stats_sokoban.npz:grids": 5, "stats_sokoban_solver.npz:grids": 21, "stats_sokoban_solver_shapes.npz:grids_8x8": 1,
                  "stats_sokoban_solver_shapes.npz:grids_20x20": 3, "stats_sokoban_solver_wide.npz:grids_20x40": 1,
                  "stats_sokoban_solver_wide.npz:grids_48x33": 3, "stats_sokoban_solver_wide.npz:grids_62x62": 1}
# which stage won, as the generator printed it (BFS, A* with balance 1, 0.5, 0): the fixture levels, the room levels
FIXTURE_STAGES, ROOM_STAGES = [28, 3, 3, 1], [68, 5, 1, 1]
N_TIE = 47  # room levels whose solution changes when `directions` is taken in reverse order


def fixture_solutions():
    """-> [(source, index, grid, moves, stage)] of tests/golden/solutions/fixture_solutions.npz"""
    z = np.load(os.path.join(SOL, "fixture_solutions.npz"))
    out, files = [], {}
    for k, (src, i) in enumerate(zip(z["source"], z["index"])):
        fname, key = str(src).split(":")
        if fname not in files:
            files[fname] = np.load(os.path.join(GOLDEN, fname))
        out.append((str(src), int(i), files[fname][key][i], z["moves"][z["offsets"][k]:z["offsets"][k + 1]].tolist(),
                    int(z["stage"][k])))
    return out


def room_file(path):
    """-> (grids, list of move lists, length, dist_win, stage, tie, solver_power)"""
    z = np.load(path)
    off = z["offsets"]
    return (z["grids"], [z["moves"][off[i]:off[i + 1]].tolist() for i in range(len(z["grids"]))], z["length"], z["dist_win"],
            z["stage"], z["tie"], int(z["solver_power"]))


def test_fixture_set_is_complete():
    assert {os.path.basename(f)[6:-4] for f in ROOMS} == ROOM_SHAPES
    assert all(os.path.getsize(f) <= 64 * 1024 for f in ROOMS + [os.path.join(SOL, "fixture_solutions.npz")])
    fx = fixture_solutions()
    assert len(fx) == 35
    counts = {}
    for src, i, grid, moves, stage in fx:
        counts[src] = counts.get(src, 0) + 1
    assert counts == FIXTURE_SOLVED
    assert [sum(f[4] == s for f in fx) for s in range(4)] == FIXTURE_STAGES
    # ... and these are ALL the solved levels of those files (the others' answers follow from the stored statistics)
    for src, n in FIXTURE_SOLVED.items():
        fname, key = src.split(":")
        z = np.load(os.path.join(GOLDEN, fname))
        assert int((z[key.replace("grids", "stats")][:, 5] > 0).sum()) == n, src
    huge = np.load(os.path.join(GOLDEN, "stats_sokoban_solver_huge.npz"))
    assert not (huge["stats"][:, 5] > 0).any()  # no solved level of more than 128 pairs is known
    stages, ties = np.zeros(4, int), 0
    for path in ROOMS:
        grids, sols, length, dist_win, stage, tie, power = room_file(path)
        shape = tuple(int(v) for v in os.path.basename(path)[6:-4].split("x"))
        assert grids.shape == (40,) + shape and grids.dtype == np.uint8 and power == 10000
        assert int((length > 0).sum()) >= 3, path
        assert np.array_equal(length > 0, stage >= 0) and np.array_equal([len(s) for s in sols], np.maximum(length, 0))
        assert np.array_equal(dist_win == 0, length > 0)
        assert np.array_equal(dist_win[length < 0], np.full(int((length < 0).sum()), shape[0] * shape[1] * sum(shape)))
        assert not tie[length <= 0].any()
        if shape[1] > 32:  # rooms across column 32
            cols = [np.flatnonzero((g != sr.SOLID).any(0)) for g in grids]
            assert sum(c.min() < 32 <= c.max() for c in cols) >= 3, path
        stages += [int((stage == s).sum()) for s in range(4)]
        ties += int(tie.sum())
    assert stages.tolist() == ROOM_STAGES and stages[0] > 0 and stages[1:].sum() > 0
    assert ties == N_TIE


def test_every_fixture_solution_replays_to_a_win():
    for src, i, grid, moves, stage in fixture_solutions():
        assert len(moves) > 0 and sr.precondition(grid), (src, i)
        assert sr.replay(grid, moves) == (True, True), (src, i)
        assert sr.replay(grid, moves[:-1])[0] is False, (src, i)  # (the search stops at the first winning node of its path)
    for path in ROOMS:
        grids, sols, length, dist_win, stage, tie, power = room_file(path)
        for i, (g, m) in enumerate(zip(grids, sols)):
            assert sr.precondition(g) == (length[i] >= 0), (path, i)
            if m:
                assert sr.replay(g, m) == (True, True), (path, i)


@pytest.mark.parametrize("path", ROOMS, ids=[os.path.basename(f)[:-4] for f in ROOMS])
def test_python_rules_reproduce_the_room_levels(path):
    """every recorded answer, move for move, with the stage that won; with `directions` reversed none of the levels the
    generator counted as telling the order apart"""
    grids, sols, length, dist_win, stage, tie, power = room_file(path)
    for i, g in enumerate(grids):
        if length[i] < 0:
            continue
        moves, dw, st = sr.solve(g, power)
        assert moves == sols[i] and dw == dist_win[i] and st == stage[i], (path, i)
        if length[i] > 0:
            rev = sr.solve(g, power, directions=sr.DIRECTIONS[::-1])[0]
            assert (rev != sols[i]) == bool(tie[i]), (path, i)


def test_python_rules_reproduce_the_fixture_solutions():
    """the solved levels of the committed solver fixtures (the large maps hold small rooms, too)"""
    for src, i, grid, moves, stage in fixture_solutions():
        got, dw, st = sr.solve(grid, 10000)
        assert got == moves and dw == 0 and st == stage, (src, i)


def test_shortcut_of_the_python_rules_changes_no_answer():
    """a BFS stage that runs dry ends the cascade (the engine's shortcut, pcgrl_sokoban.h sk_cascade): the three A* stages it
    skips would return the same dist-win"""
    grids, sols, length, dist_win, stage, tie, power = room_file(os.path.join(SOL, "rooms_8x8.npz"))
    n = 0
    for i in np.flatnonzero(length == 0)[:12]:
        assert sr.solve(grids[i], power, shortcut=False) == ([], int(dist_win[i]), -1)
        n += 1
    assert n == 12


def test_solutions_header_symbols_exported_and_bound():
    from control_pcgrl_amd import _lib
    _lib.build()
    header = open(os.path.join(ROOT, "include", "pcgrl_amd_solutions.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z_]+)\s*\(", header))
    assert declared == {"pcgrl_solution_capacity", "pcgrl_solutions", "pcgrl_solutions_for_grids"}
    assert set(_lib.SOLUTIONS_SYMBOLS) == declared
    assert not declared & (set(_lib.SYMBOLS) | set(_lib.CODES_SYMBOLS) | set(_lib.ASYNC3D_SYMBOLS) | set(_lib.PATHS_SYMBOLS))
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)
        assert fn.argtypes == _lib.SOLUTIONS_SYMBOLS[name][1] and fn.restype == _lib.SOLUTIONS_SYMBOLS[name][0], name
    for name, params in re.findall(r"\b(pcgrl_[a-z_]+)\s*\(([^)]*)\)\s*;", header):
        assert len(params.split(",")) == len(_lib.SOLUTIONS_SYMBOLS[name][1]), name
    assert "solutions/pcgrl_k_solutions.hip" in _lib.UNITS and "solutions/pcgrl_solutions.h" in _lib.HEADERS


def test_solution_entry_points_refuse_bad_arguments_by_name():
    """the checks that come before any HIP call: reachable without a device"""
    from control_pcgrl_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    assert L.pcgrl_solution_capacity(None) == -1
    for args in ((None, 4, p, p, None, None), (None, 4, None, None, None, None), (None, 0, p, p, p, None)):
        assert L.pcgrl_solutions(*args) == 1
        assert b"pcgrl_solutions:" in L.pcgrl_last_error()
    for args in ((None, 1, p, 4, p, p, None, None), (None, 1, None, 4, None, None, None, None), (None, 1, p, 0, p, p, None, None),
                 (None, -1, p, 4, p, p, None, None), (None, 0, p, 4, p, p, None, None)):
        assert L.pcgrl_solutions_for_grids(*args) == 1
        assert b"pcgrl_solutions_for_grids:" in L.pcgrl_last_error()


def test_step_kernels_are_the_profiled_ones():
    """the feature lives in csrc/solutions/ and the host unit: the sources of the step kernels -- pcgrl_sokoban.h among them -- are
    the bytes profiles/r06_summary.json was taken on"""
    import bench
    s = json.load(open(os.path.join(ROOT, "profiles", "r06_summary.json")))
    assert s["kernel_sources_sha16"] == bench.kernel_sources_sha16()
