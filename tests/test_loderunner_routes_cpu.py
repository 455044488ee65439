"""The routes behind a Lode Runner level's path-length (include/pcgrl_amd_loderunner_routes.h) on the host: the plain-Python
rules reproduce every list recorded from the reference (tools/gen_golden_loderunner_routes.py ->
tests/golden/loderunner_routes), the fixture set holds the shapes and the cases it has to, the ABI symbol is declared, listed
and bound, its argument checks answer before any HIP call, and the Python surface is in place.  No GPU needed."""
import ctypes as C
import glob
import inspect
import os
import re

import numpy as np
import pytest

import loderunner_routes_expect as X
import loderunner_rules as R
from conftest import GOLDEN
from control_pcgrl_amd import _lib, loderunner

DIR = os.path.join(GOLDEN, "loderunner_routes")
FIXTURES = sorted(glob.glob(os.path.join(DIR, "*.npz")))
SHAPES = {(1, 5), (2, 1), (4, 4), (5, 7), (8, 12), (16, 32)}


def fixture_id(path):
    return os.path.basename(path)[:-4]


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_rules_reproduce_every_recorded_list_and_action(path):
    z = np.load(path)  # (allow_pickle is off: arrays only)
    assert list(z["move_names"]) == R.MOVE_NAMES
    assert len(z["path_off"]) == len(z["act_off"]) == 2 * len(z["pair_level"]) + 1
    assert z["path_cells"].dtype == np.int16 and z["path_actions"].dtype == np.int16
    seen = 0
    for i, m in enumerate(z["grids"]):
        pairs = X.pairs_of_fixture(z, i)
        assert pairs == X.pairs_of_rules(m), (fixture_id(path), i)
        seen += len(pairs)
        stats, rec = R.get_stats(m)
        for j, to_goal, to_start in pairs:  # a recorded list is a walk by its recorded moves, between the landing cell and the gold
            assert rec["state"][j] == R.BY_OWN_SEARCHES and rec["dist"][j] == len(to_goal[0])
            assert to_goal[0][0] == to_start[0][-1] == rec["golds"][j] and to_goal[0][-1] == to_start[0][0] == rec["landing"]
            for cells, moves in (to_goal, to_start):
                for k, a in enumerate(moves):  # listed from the goal back: moves[k] led from cells[k + 1] to cells[k]
                    assert (cells[k + 1][0] + R.DELTA[a][0], cells[k + 1][1] + R.DELTA[a][1]) == cells[k]
        if rec is not None:
            assert sum(len(a[0]) for _, a, _ in pairs) == stats[4]
    assert seen == len(z["pair_level"])


def test_fixture_set_holds_the_shapes_and_the_cases():
    assert {np.load(f)["grids"].shape[1:] for f in FIXTURES} == SHAPES and len(FIXTURES) == 7
    assert all(os.path.getsize(f) <= 100 * 1024 for f in FIXTURES)
    got = set()
    for f in FIXTURES:
        z = np.load(f)
        H, W = z["grids"].shape[1:]
        for i, m in enumerate(z["grids"]):
            pairs = X.pairs_of_fixture(z, i)
            got |= {"index 32" for j, _, _ in pairs if j >= 32}
            got |= {"asymmetric" for _, a, b in pairs if b[0] != a[0][::-1]}
            got |= {"long" for _, a, b in pairs if max(len(a[0]), len(b[0])) > 64}
            got |= {"cell 256" for _, a, b in pairs for r, c in a[0] + b[0] if (H, W) == (16, 32) and r * W + c >= 256}
            got |= {R.MOVE_NAMES[k] for _, a, b in pairs for k in a[1] + b[1]}
            if pairs:
                state = R.get_stats(m)[1]["state"]
                first = {j // 32 for j, _, _ in pairs}
                got |= {"state 2 in a counted gold's round" for j, s in enumerate(state) if s == R.ON_ANOTHER_PATH and j // 32 in first}
    assert got == {"index 32", "asymmetric", "long", "cell 256", "state 2 in a counted gold's round"} | set(R.MOVE_NAMES)


def test_serpentine_has_one_long_way():
    m = X.serpentine(16, 32)
    (j, to_goal, to_start), = X.pairs_of_rules(m)
    assert j == 0 and len(to_goal[0]) == len(to_start[0]) == 8 * 32 + 7 > 64 and to_start[0] == to_goal[0][::-1]
    z = np.load(os.path.join(DIR, "h16w32.npz"))
    i = list(z["kind"]).index("serpentine")
    assert np.array_equal(z["grids"][i], m)


def test_header_table_and_prototype_agree():
    _lib.build()
    assert "loderunner/pcgrl_k_loderunner_routes.hip" in _lib.UNITS and "loderunner/pcgrl_loderunner_routes.h" in _lib.HEADERS
    for f in ("loderunner/pcgrl_k_loderunner_routes.hip", "loderunner/pcgrl_loderunner_routes.h"):
        assert os.path.exists(os.path.join(_lib.CSRC, f))
    header = re.sub(r"/\*.*?\*/", "", open(_lib.LODERUNNER_ROUTES_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(", header))
    assert declared == {"pcgrl_loderunner_routes"} == set(_lib.LODERUNNER_ROUTES_SYMBOLS)
    L = _lib.lib()
    res, args = _lib.LODERUNNER_ROUTES_SYMBOLS["pcgrl_loderunner_routes"]
    fn = L.pcgrl_loderunner_routes  # (exported by the library)
    assert fn.argtypes == args and fn.restype == res == C.c_int
    (params,) = re.findall(r"\bpcgrl_loderunner_routes\s*\(([^)]*)\)\s*;", header)
    params = [" ".join(p.split()) for p in params.split(",")]
    assert len(params) == len(args) == 19
    # evaluate's arguments in evaluate's order, with route_cap behind gold_cap and the route outputs before d_error
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["cfg", "n", "d_grids", "d_workspace", "workspace_bytes", "gold_cap", "route_cap", "d_stats", "d_loss", "d_play",
                     "d_gold_state", "d_gold_dist", "d_gold_off", "d_gold_back", "d_coords", "d_moves", "d_tour_len", "d_error",
                     "stream"]
    for p, a in zip(params, args):
        want = C.c_int32 if p.startswith("int32_t ") and "*" not in p else (C.c_int64 if p.startswith("int64_t ") else None)
        if want is not None:
            assert a is want, p
        else:
            assert "*" in p and a in (C.c_void_p, C.POINTER(_lib.PcgrlLoderunnerConfig)), p
    # plain HIP C++, and the rules are written once: the routes kernel composes the evaluator's device functions
    src = open(os.path.join(_lib.CSRC, "loderunner/pcgrl_loderunner_routes.h")).read()
    assert "asm" not in src and "lr_evaluate_level(L, H, W, slot, r, hook)" in src and "lr_store_level(" in src
    assert "lr_search(" not in src and "while (open" not in src  # no second search, no second open list
    unit = open(os.path.join(_lib.CSRC, "loderunner/pcgrl_k_loderunner_routes.hip")).read()
    assert "#define PCGRL_LR_DEVICE_ONLY" in unit
    # the other tables are as they were
    assert set(_lib.LODERUNNER_SYMBOLS) == {"pcgrl_loderunner_workspace_bytes", "pcgrl_loderunner_evaluate"}
    assert set(_lib.LODERUNNER_MEASURES_SYMBOLS) == {"pcgrl_loderunner_measures_for_grids", "pcgrl_loderunner_diversity_scratch_bytes",
                                                    "pcgrl_loderunner_diversity_for_grids"}
    others = [table for _, table in _lib.ABI if table is not _lib.LODERUNNER_ROUTES_SYMBOLS]
    assert len(others) == len(_lib.ABI) - 1
    assert not any(declared & set(o) for o in others)
    assert _lib.ABI[17][1] is _lib.LODERUNNER_ROUTES_SYMBOLS  # the tables before this one are as they were
    assert [len(table) for _, table in _lib.ABI[:17]] == [49, 5, 1, 3, 3, 8, 6, 2, 11, 5, 6, 3, 6, 2, 5, 2, 3]
    assert b"0.7.0" in L.pcgrl_version()


def test_every_argument_check_is_answered_without_a_device():
    L = _lib.lib()
    # pointers that are never dereferenced: every call below is refused before any HIP call
    grids, ws, stats, coords = 0x1000, 0x2000, 0x3000, 0x4000
    need = L.pcgrl_loderunner_workspace_bytes(2, 8, 12)

    def call(cfg, n=2, g=grids, w=ws, wb=need, cap=8, rcap=16, st=stats, co=coords):
        return L.pcgrl_loderunner_routes(C.byref(cfg) if cfg is not None else None, n, g, w, wb, cap, rcap, st, None, None, None,
                                         None, None, None, co, None, None, None, None)

    ok = loderunner.loderunner_config((8, 12))
    EINVAL, EUNSUPPORTED = 1, 2
    # everything pcgrl_loderunner_evaluate refuses
    assert call(None) == EINVAL
    assert call(ok, g=None) == EINVAL and call(ok, st=None) == EINVAL
    assert call(ok, n=0) == EINVAL and call(ok, n=-3) == EINVAL
    assert b"pcgrl_loderunner_routes:" in L.pcgrl_last_error()
    assert call(ok, cap=-1) == EINVAL and b"gold_cap" in L.pcgrl_last_error()
    assert call(ok, w=None) == EINVAL and call(ok, wb=need - 1) == EINVAL and call(ok, w=ws + 2) == EINVAL
    assert b"workspace" in L.pcgrl_last_error()
    # and the route buffer
    assert call(ok, rcap=-1) == EINVAL and b"route_cap must not be negative" in L.pcgrl_last_error()
    assert call(ok, rcap=1, co=None) == EINVAL and b"d_coords" in L.pcgrl_last_error()
    for shape in ((0, 12), (17, 12), (8, 0), (8, 33)):
        assert call(loderunner.loderunner_config(shape)) == EUNSUPPORTED, shape
        assert b"1..16 rows and 1..32 columns" in L.pcgrl_last_error()


def test_python_surface_and_defaults():
    import control_pcgrl_amd
    ev = loderunner.LodeRunnerEvaluator
    sig = inspect.signature(ev.routes).parameters
    assert list(sig) == ["self", "grids", "gold_cap", "route_cap", "moves"]
    assert sig["gold_cap"].default == 32 and sig["route_cap"].default is None and sig["moves"].default is False
    assert list(inspect.signature(ev.split_routes).parameters) == ["result", "i"]
    assert isinstance(inspect.getattr_static(ev, "split_routes"), staticmethod)  # a host-side helper: no evaluator needed
    # what was there keeps its signature
    assert list(inspect.signature(ev.evaluate).parameters) == ["self", "grids", "gold_cap"]
    assert list(inspect.signature(ev.measures).parameters) == ["self", "grids", "entropy"]
    assert list(inspect.signature(ev.diversity).parameters) == ["self", "grids", "group", "pairwise"]
    assert list(inspect.signature(ev.behaviour).parameters) == ["self", "grids", "names"]
    assert list(inspect.signature(ev.check_errors).parameters) == ["self"]
    assert "stepping Lode Runner environments is not built" in loderunner.__doc__ and "routes" in loderunner.__doc__
    assert "routes()" in control_pcgrl_amd.__doc__
    assert control_pcgrl_amd.__version__ == "0.7.0"


def test_split_routes_on_a_result_assembled_by_hand():
    split = loderunner.LodeRunnerEvaluator.split_routes
    # level 0: golds 0 (state 2), 1 (counted: 3 cells out, 4 back) and 3 (counted: 2 out, 2 back); level 1: nothing
    tour = [(5, 0), (5, 1), (5, 2), (5, 2), (4, 2), (4, 1), (5, 0), (5, 0), (6, 1), (6, 1), (5, 0)]
    coords = np.full((2, 16, 2), -1, np.int16)
    coords[0, :len(tour)] = tour
    result = {"coords": coords, "tour_len": np.array([11, 0], np.int32),
              "gold_state": np.array([[2, 1, 0, 1, -1], [0, 3, -1, -1, -1]], np.int8),
              "gold_dist": np.array([[0, 3, 0, 2, 0], [0] * 5], np.int16),
              "gold_off": np.array([[-1, 0, -1, 7, -1], [-1] * 5], np.int32),
              "gold_back": np.array([[0, 4, 0, 2, 0], [0] * 5], np.int16)}
    assert split(result, 0) == [((5, 2), tour[0:3], tour[3:7]), ((6, 1), tour[7:9], tour[9:11])]
    assert split(result, 1) == []
    # the same from the rules' pairs, through the expected arrays
    m = np.load(os.path.join(DIR, "stock_gold.npz"))["grids"]
    pairs = [X.pairs_of_rules(g) for g in m]
    want = X.expect(pairs, 48, 256)
    for i, g in enumerate(m):
        stats, rec = R.get_stats(g)
        want_i = {k: v[i:i + 1] for k, v in want.items()}
        want_i["gold_state"] = np.array([(rec["state"] + [-1] * 48)[:48]], np.int8)
        want_i["gold_dist"] = np.array([(rec["dist"] + [0] * 48)[:48]], np.int16)
        assert split(want_i, 0) == X.split(pairs[i])
    # a result that the caps cut is refused, not silently shortened
    with pytest.raises(ValueError):
        split({**result, "coords": coords[:, :10]}, 0)
    with pytest.raises(ValueError):
        split({k: (v[:, :3] if k.startswith("gold") else v) for k, v in result.items()}, 0)
    with pytest.raises(ValueError):
        split({k: v for k, v in result.items() if k != "gold_off"}, 0)
