"""The 3-D holey dungeon and maze levels without a device: the plain-Python rules (tests/mc3d_holey_rules.py) against the fixtures
recorded from the reference (tests/golden/mc3d_holey, tools/gen_golden_mc3d_holey.py), the cases the fixtures hold, the wrong
rules, the holes against the recorded lists, the loss tables, the header against the symbol list, every refusal of the C ABI
(made before any HIP call) and of the Python class, and archive_for's bounds."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import mc3d_holey_levels as Lv
import mc3d_holey_rules as R
from control_pcgrl_amd import _lib, archive, mc3d_holey, problems

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mc3d_holey")
PROBLEMS = ("dungeon", "maze")
SYMBOLS = {"pcgrl_mc3d_holey_workspace_bytes", "pcgrl_mc3d_holey_evaluate"}


def load(problem):
    z = np.load(os.path.join(GOLDEN, problem + ".npz"))
    levels, at = [], 0
    for i, shape in enumerate(z["shapes"]):
        size = int(np.prod(shape))
        rec = {"name": str(z["names"][i]), "grid": z["grids"][at:at + size].reshape(shape), "holes": z["holes"][i],
               "stats": z["stats"][i].tolist(), "leg_len": z["leg_len"][i].tolist()}
        for k in ("route", "route2", "overlay", "overlay2"):
            rec[k] = [tuple(int(v) for v in t) for t in z[k][z[k + "_off"][i]:z[k + "_off"][i + 1]]]
        levels.append(rec)
        at += size
    return z, levels


def agrees(lv, res):
    return (lv["stats"] == res["stats"] and lv["route"] == res["route"] and lv["route2"] == res["route2"]
            and lv["overlay"] == sorted(res["overlay"]) and lv["overlay2"] == sorted(res["overlay2"])
            and lv["leg_len"] == list(res["leg_len"]))


@pytest.mark.parametrize("problem", PROBLEMS)
def test_rules_equal_fixtures(problem):
    z, levels = load(problem)
    assert len(levels) >= 20 and os.path.getsize(os.path.join(GOLDEN, problem + ".npz")) <= 100 * 1024
    for lv in levels:
        res = R.evaluate(problem, lv["grid"], lv["holes"])
        assert agrees(lv, res), lv["name"]
        assert res["error"] == 0 and (problem == "maze" or len(res["route"]) == sum(res["leg_len"]))


@pytest.mark.parametrize("problem", PROBLEMS)
def test_fixtures_show_the_cases(problem):
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "..", "tools"))
    import gen_golden_mc3d_holey as G
    _, levels = load(problem)
    shown = set()
    for lv in levels:
        shown |= G.cases_of(problem, lv["grid"], lv["holes"], R.evaluate(problem, lv["grid"], lv["holes"]))
    assert not G.NEEDED[problem] - shown, sorted(G.NEEDED[problem] - shown)


def test_wrong_rules_fail_some_fixture():
    fails = dict.fromkeys((name for name, _ in R.WRONG_RULES), 0)
    for problem in PROBLEMS:
        for lv in load(problem)[1]:
            for name, kw in R.WRONG_RULES:
                fails[name] += not agrees(lv, R.evaluate(problem, lv["grid"], lv["holes"], **kw))
    assert all(fails.values()), fails


def test_holes_against_the_recorded_lists():
    z, _ = load("maze")
    for shape in ((3, 3, 3), (3, 4, 5)):
        key = "%dx%dx%d" % shape
        mine = mc3d_holey.all_holes(shape)
        assert mine.dtype == np.int32 and np.array_equal(mine, z["all_holes_" + key]) and np.array_equal(mine, R.all_holes(shape))
        assert np.array_equal(mc3d_holey.fixed_holes(shape), z["fixed_holes_" + key])
        assert all(mc3d_holey.hole_ok(p[0], shape) and mc3d_holey.hole_ok(p[1], shape) for p in mine)
    assert mc3d_holey.fixed_holes((7, 7, 7)).tolist() == [[1, 0, 7], [2, 8, 1]]
    assert len(mc3d_holey.all_holes((7, 7, 7))) == len(R.all_holes((7, 7, 7))) > 20000
    for foot in ([0, 2, 0], [7, 2, 0], [1, 0, 0], [1, 8, 8], [1, 3, 3], [1, 2, 9], [-1, 2, 0], [1, 9, 3]):
        assert not mc3d_holey.hole_ok(foot, (7, 7, 7)) and not R.hole_ok(foot, (7, 7, 7)), foot
    for foot in ([1, 2, 0], [6, 7, 8], [3, 0, 1], [3, 8, 7]):
        assert mc3d_holey.hole_ok(foot, (7, 7, 7)) and R.hole_ok(foot, (7, 7, 7)), foot


def test_the_loss_tables():
    # derived from the code: minecraft_3D_maze_prob.py:33-35 freezes 15^3; :46-50 the longest path
    per_floor = math.ceil(15 / 2) * 15 + math.floor(15 / 2)
    assert per_floor == 127 and 2 * (15 // 3) * per_floor == 1270 == R.MAX_PATH
    d, m = mc3d_holey.mc3d_holey_spec("dungeon", (7, 7, 7)), mc3d_holey.mc3d_holey_spec("maze", (3, 4, 5))
    assert d.stat_keys == R.STAT_KEYS["dungeon"] and m.stat_keys == R.STAT_KEYS["maze"]
    assert d.tile_types == ["AIR", "DIRT", "CHEST", "SKULL", "PUMPKIN"] and m.tile_types == ["AIR", "DIRT"]
    assert d.static_trgs == {"regions": 1, "path-length": 12700, "chests": 1, "enemies": (2, 5), "nearest-enemy": (5, 635),
                             "n_jump": (2, 5)} == R.TARGETS["dungeon"]
    assert m.static_trgs == {"regions": 1, "path-length": 12700, "connected-path-length": 12700, "n_jump": 5} == R.TARGETS["maze"]
    assert d.default_weights == {"regions": 0, "path-length": 100, "chests": 300, "enemies": 100, "nearest-enemy": 200,
                                 "n_jump": 100} == R.WEIGHTS["dungeon"]
    assert m.default_weights == {"regions": 0, "path-length": 100, "connected-path-length": 120, "n_jump": 150} == R.WEIGHTS["maze"]
    assert d.cond_bounds == R.BOUNDS["dungeon"] and m.cond_bounds == R.BOUNDS["maze"]
    assert d.cond_bounds["regions"] == (0, 1688) and d.cond_bounds["chests"] == (0, 843) and m.cond_bounds["path-length"] == (0, 1272)
    assert mc3d_holey.mc3d_holey_spec("maze", (16, 16, 16)).static_trgs == m.static_trgs  # whatever the map's size
    cfg = mc3d_holey.mc3d_holey_config("dungeon", (7, 7, 7))
    assert [cfg.trg_lo[i] for i in range(6)] == [1, 12700, 1, 2, 5, 2] and [cfg.trg_hi[i] for i in range(6)] == [1, 12700, 1, 4, 634, 4]
    assert (cfg.problem, cfg.z, cfg.y, cfg.x) == (0, 7, 7, 7) and [cfg.weight[i] for i in range(6)] == [0, 100, 300, 100, 200, 100]
    cfg = mc3d_holey.mc3d_holey_config("maze", (3, 4, 5), weights={"n_jump": 2.5})
    assert (cfg.problem, cfg.z, cfg.y, cfg.x) == (1, 3, 4, 5) and [cfg.weight[i] for i in range(4)] == [0, 0, 0, 2.5]
    with pytest.raises(ValueError):
        mc3d_holey.mc3d_holey_config("maze", (3, 4, 5), weights={"chests": 1})
    # hand-computed losses: the tuple targets are the integers of arange(lo, hi)
    assert R.loss_of("dungeon", [1, 0, 0, 0, 0, 0]) == -(12700 * 100 + 300 + 2 * 100 + 5 * 200 + 2 * 100)
    assert R.loss_of("dungeon", [3, 20, 1, 4, 634, 4]) == -(12680 * 100)
    assert R.loss_of("dungeon", [1, 20, 2, 5, 635, 5]) == -(12680 * 100 + 300 + 100 + 200 + 100)
    assert R.loss_of("maze", [1, 8, -1, 0]) == -(12692 * 100 + 12701 * 120 + 5 * 150)
    assert R.target_term(3.0, (2, 5), 7) == 0.0 and R.target_term(7.0, 5, 2) == -4.0
    assert problems.target_interval((5, 635)) == (5.0, 634.0)


def test_header_units_symbols_and_config():
    _lib.build()
    unit, header = "mc3d_holey/pcgrl_k_mc3d_holey.hip", "mc3d_holey/pcgrl_mc3d_holey.h"
    assert unit in _lib.UNITS and header in _lib.HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, unit)) and os.path.exists(os.path.join(_lib.CSRC, header))
    text = re.sub(r"/\*.*?\*/", "", open(_lib.MC3D_HOLEY_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(", text))
    assert declared == SYMBOLS == set(_lib.MC3D_HOLEY_SYMBOLS)
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)
        want = _lib.MC3D_HOLEY_SYMBOLS[name]
        assert fn.argtypes == want[1] and fn.restype == want[0], name
    for name, params in re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        assert len(params.split(",")) == len(_lib.MC3D_HOLEY_SYMBOLS[name][1]), name
    assert C.sizeof(_lib.PcgrlMc3dHoleyConfig) == 4 * 4 + 3 * 6 * 8 and _lib.PcgrlMc3dHoleyConfig.weight.offset == 16
    assert _lib.PCGRL_MC3D_HOLEY_MAX_STATS == 6 and _lib.PCGRL_MC3D_HOLEY_PLAY == 12 == R.PLAY
    m = re.search(r"typedef struct pcgrl_mc3d_holey_config \{(.*?)\} pcgrl_mc3d_holey_config;", text, flags=re.S)
    fields = re.findall(r"\b([a-z_]+)\s*(?:\[[A-Z0-9_]+\])?\s*[,;]", m.group(1))
    assert fields == [f[0] for f in _lib.PcgrlMc3dHoleyConfig._fields_]
    # the kernel restates the move rule: nothing of the 3-D maze's kernels is included, so their code cannot change
    src = open(os.path.join(_lib.CSRC, header)).read()
    assert "pcgrl_kernels3d.h\"" not in src and "#include \"" not in src
    assert "asm" not in src.replace("namespace", "")
    assert "H3_MAX_CELLS = H3_B * H3_B * H3_B" in src and 18 ** 3 < 1 << 13 and 3 * 18 ** 3 + 3 < 1 << 15


def test_workspace_bytes():
    L = _lib.lib()
    ws = L.pcgrl_mc3d_holey_workspace_bytes

    def slot(z, y, x):
        cells = (z + 2) * (y + 2) * (x + 2)
        q = 64
        while q < 8 * cells:
            q *= 2
        state = 0 if cells <= 1024 else 4 * ((2 * cells + 15) // 16 * 16) + (cells + 15) // 16 * 16
        return 2 * (q * 8 + state)

    assert ws(1, 7, 7, 7) == slot(7, 7, 7) == 2 * 8192 * 8 == 131072
    assert ws(1, 8, 8, 8) == 2 * 8192 * 8 and ws(1, 8, 8, 9) == slot(8, 8, 9) > 2 * 16384 * 8  # past 1024 cells: the state too
    assert ws(5, 15, 15, 15) == 5 * slot(15, 15, 15) and ws(1, 16, 16, 16) == slot(16, 16, 16) == 2 * (65536 * 8 + 4 * 11664 + 5840)
    assert all(slot(*s) % 16 == 0 for s in ((3, 3, 3), (3, 4, 5), (9, 9, 9), (16, 3, 16)))
    assert "128 KiB" in mc3d_holey.Mc3dHoleyEvaluator.__doc__ and slot(7, 7, 7) == 128 * 1024
    for blocks in (0, -1):
        assert ws(blocks, 7, 7, 7) < 0 and b"pcgrl_mc3d_holey_workspace_bytes: blocks must be at least 1" in L.pcgrl_last_error()
    for shape in ((2, 7, 7), (7, 17, 7), (7, 7, 0), (-3, 7, 7), (7, 7, 17)):
        assert ws(1, *shape) < 0 and b"pcgrl_mc3d_holey_workspace_bytes: interiors of 3..16" in L.pcgrl_last_error()


def test_abi_argument_checks_need_no_device():
    L = _lib.lib()
    # pointers that are never dereferenced: every call below is refused before any HIP call
    grids, holes, stats, wsp = 0x1000, 0x2000, 0x3000, 0x10000
    EINVAL, EUNSUPPORTED = 1, 2
    who = b"pcgrl_mc3d_holey_evaluate:"

    def call(cfg, n=2, g=grids, h=holes, ws=wsp, ws_bytes=1 << 40, cap=8, st=stats):
        return L.pcgrl_mc3d_holey_evaluate(C.byref(cfg) if cfg is not None else None, n, g, h, ws, ws_bytes, cap, st,
                                           *([None] * 11))

    ok = mc3d_holey.mc3d_holey_config("dungeon", (7, 7, 7))
    for kw in (dict(cfg=None), dict(cfg=ok, g=None), dict(cfg=ok, h=None), dict(cfg=ok, st=None), dict(cfg=ok, n=0),
               dict(cfg=ok, n=-3)):
        assert call(**kw) == EINVAL and who + b" bad arguments" in L.pcgrl_last_error(), kw
    assert call(ok, cap=-1) == EINVAL and who + b" route_cap must not be negative" in L.pcgrl_last_error()
    for problem in (2, -1):
        bad = mc3d_holey.mc3d_holey_config("maze", (7, 7, 7))
        bad.problem = problem
        assert call(bad) == EINVAL and who + b" problem must be 0 (dungeon) or 1 (maze)" in L.pcgrl_last_error()
    need = L.pcgrl_mc3d_holey_workspace_bytes(1, 7, 7, 7)
    for kw in (dict(ws=None), dict(ws=wsp + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(ok, **kw) == EINVAL and who + b" the workspace is null, not 16-byte aligned or smaller" in L.pcgrl_last_error()
    for shape in ((2, 7, 7), (7, 17, 7), (7, 7, 0), (17, 17, 17), (-1, 4, 4)):
        for problem in PROBLEMS:
            assert call(mc3d_holey.mc3d_holey_config(problem, shape)) == EUNSUPPORTED, shape
            assert who + b" interiors of 3..16 cells along each axis only" in L.pcgrl_last_error()


def test_python_refusals():
    E = mc3d_holey.Mc3dHoleyEvaluator
    for shape in ((2, 7, 7), (7, 17, 7), (7, 7, 0)):
        with pytest.raises(NotImplementedError):
            E("maze", shape)
    with pytest.raises(ValueError, match="no CPU fallback"):
        E("dungeon", (7, 7, 7), device="cpu", max_blocks=1)
    with pytest.raises(ValueError, match="3-D"):
        E("dungeon", (7, 7))
    with pytest.raises(ValueError, match="'dungeon' or 'maze'"):
        E("zelda", (7, 7, 7))
    with pytest.raises(ValueError, match="max_blocks"):
        E("maze", (7, 7, 7), max_blocks=0)
    with pytest.raises(ValueError):
        mc3d_holey.mc3d_holey_spec("binary")
    import control_pcgrl_amd
    assert control_pcgrl_amd.Mc3dHoleyEvaluator is E and control_pcgrl_amd.mc3d_holey_spec is mc3d_holey.mc3d_holey_spec
    assert control_pcgrl_amd.fixed_holes is mc3d_holey.fixed_holes and control_pcgrl_amd.all_holes is mc3d_holey.all_holes
    assert "minecraft_3D_dungeon_holey" not in problems.PROBLEMS  # evaluated, not stepped: the engine does not know it


def test_archive_for_bounds():
    for problem in PROBLEMS:
        spec = mc3d_holey.mc3d_holey_spec(problem, (16, 16, 16))
        names = ["path-length", "n_jump", "regions"]
        dims, bounds = archive.archive_shape(spec, names, bins=9)
        assert dims == [9, 9, 9] and bounds == [tuple(float(v) for v in R.BOUNDS[problem][k]) for k in names]
        with pytest.raises(Exception, match="brightness"):
            archive.archive_shape(spec, ["brightness"])
    assert 16 ** 3 <= archive.MAX_MAP_BYTES  # the largest interior fits an archive row
    # a stand-in with the evaluator's surface: archive_for asks the evaluator which names it serves before any device work
    stub = mc3d_holey.Mc3dHoleyEvaluator.__new__(mc3d_holey.Mc3dHoleyEvaluator)
    stub.stat_keys, stub.problem = list(R.STAT_KEYS["maze"]), "maze"
    with pytest.raises(NotImplementedError, match="2-D"):
        archive.archive_for(stub, ["emptiness"])
    with pytest.raises(ValueError, match="chests"):
        archive.archive_for(stub, ["chests"])


def test_generators_and_hand_levels():
    # the sets the GPU tests and the bench use connect in at least half of their levels, from the rules alone
    for problem in PROBLEMS:
        for shape, n in (((3, 3, 3), 24), ((3, 4, 5), 24), ((7, 7, 7), 24)):
            grids, holes = Lv.structured_set(problem, shape, n, seed=11)
            assert all(R.hole_ok(h[0], shape) and R.hole_ok(h[1], shape) for h in holes)
            res = [R.evaluate(problem, grids[i], holes[i]) for i in range(n)]
            assert 2 * sum(Lv.connected(problem, r) for r in res) >= n, (problem, shape)
            again = Lv.structured_set(problem, shape, n, seed=11)
            assert np.array_equal(again[0], grids) and np.array_equal(again[1], holes)
    by = {name: R.evaluate("dungeon", g, h) for name, g, h in Lv.hand_levels("dungeon")}
    assert by["enemy-adjacent"]["stats"][4] == 2 and by["two-enemies-equal"]["play"][8:11] == [2, 1, 1]
    assert by["chest-midair"]["leg_len"] == [0, 6] and by["chest-no-headroom"]["play"][3:5] == [0, 1]
    assert by["isolated-exit-hole"]["stats"][0] == 2 and by["items-split-air"]["stats"][0] == 2
    # a refused hole and an unknown tile
    g, h = Lv.hand_levels("maze")[0][1:]
    bad = R.evaluate("maze", g, np.array([[1, 0, 0], [1, 3, 6]]))
    assert bad["error"] == R.ERR_HOLE and bad["stats"] == [-1] * 4 and bad["loss"] == -math.inf and not bad["route"]
    g2 = g.copy()
    g2[0, 0, 0] = 3
    assert R.evaluate("maze", g2, h)["error"] == R.ERR_TILE
