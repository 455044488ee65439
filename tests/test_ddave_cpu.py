"""Dangerous Dave levels, the parts that need no GPU: the plain-Python rules (tests/ddave_rules.py) against the fixtures recorded
from the reference (tests/golden/ddave, tools/gen_golden_ddave.py), the cases the fixtures hold, the restated reward on
hand-computed cases, the header, the symbols and the config struct, the argument checks of the C ABI
(include/pcgrl_amd_ddave.h: made before any HIP call, so they answer without a device), the workspace sizes, the Python surface,
and what stays outside the engine."""
import ctypes as C
import glob
import inspect
import math
import os
import re

import numpy as np
import pytest

import ddave_levels as DL
import ddave_rules as R
import measures_numpy as mn
from conftest import GOLDEN
from control_pcgrl_amd import _lib, ddave, problems
from control_pcgrl_amd.vec_env import build_config

DIR = os.path.join(GOLDEN, "ddave")
FILES = sorted(glob.glob(os.path.join(DIR, "dd_*.npz")))
SETS = [(7, 11, 5000)] + [(h, w, p) for h, w in ((1, 1), (1, 3), (2, 3), (3, 4), (5, 13), (16, 32)) for p in (1, 2, 50, 500)]
MEAS_SHAPES = [(1, 1), (1, 32), (16, 1), (5, 2), (5, 13), (7, 11), (16, 32)]
SYMBOLS = {"pcgrl_ddave_workspace_bytes", "pcgrl_ddave_evaluate", "pcgrl_ddave_measures_for_grids",
           "pcgrl_ddave_diversity_scratch_bytes", "pcgrl_ddave_diversity_for_grids"}


def _bits(values):
    return np.asarray([float(v) for v in values], np.float64).view(np.uint64)


def _load(h, w, power):
    return np.load(os.path.join(DIR, f"dd_{h}x{w}_p{power}.npz"))


def test_fixture_set_is_complete():
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(DIR, "*.npz")))
    assert names == sorted([f"dd_{h}x{w}_p{p}.npz" for h, w, p in SETS] + [f"meas_{h}x{w}.npz" for h, w in MEAS_SHAPES])
    assert max(os.path.getsize(os.path.join(DIR, f)) for f in names) <= 100 * 1024
    for (h, w, p), f in zip(SETS, (os.path.join(DIR, f"dd_{h}x{w}_p{p}.npz") for h, w, p in SETS)):
        z = np.load(f)  # (allow_pickle is off: arrays only)
        n = len(z["grids"])
        assert z["grids"].dtype == np.uint8 and z["grids"].shape[1:] == (h, w) and z["grids"].max() <= 6 and int(z["power"]) == p
        assert list(z["stat_keys"]) == R.STAT_KEYS and z["stats"].shape == (n, 11) and z["stats"].dtype == np.int32
        assert z["stage_iters"].shape == z["stage_won"].shape == (n, 4) and z["stage_node"].shape == (n, 4, 3)
        assert z["play"].shape == (n, 12) and z["length"].shape == (n,) and z["moves"].shape[0] == n and len(z["names"]) == n
        assert z["moves"].shape[1] == max(1, z["length"].max())  # every action of every level is recorded
        m = len(z["rew_new"])
        assert z["rew_old"].shape == (m, 11) and z["rew_bits"].shape == z["rew_bits_custom"].shape == (m,)
        assert z["over"].shape == z["over_custom"].shape == (m,) and z["custom_weights"].shape == (10,)
        assert (z["grids"] == DL.DIAMOND).reshape(n, -1).sum(1).max() <= R.MAX_DIAMONDS
    assert len(_load(7, 11, 5000)["grids"]) >= 200


def test_fixtures_show_the_cases():
    won, budget, emptied, negative, pre = set(), 0, 0, 0, set()
    for h, w, p in SETS:
        z = _load(h, w, p)
        st, pl = z["stats"], z["play"]
        won |= set(pl[:, 0][pl[:, 0] > 0].tolist())
        budget += int(((pl[:, 0] == 0) & (pl[:, 4] == p)).sum())
        emptied += int(((pl[:, 0] == 0) & (pl[:, 4] < p)).sum())
        negative += int((st[:, 9] < 0).sum())
        for i, s in enumerate(st):
            one = [s[j] == 1 for j in (0, 2, 4, 6)]
            if sum(one) == 3:
                pre.add((("player", "exit", "key", "regions")[one.index(False)], int(s[(0, 2, 4, 6)[one.index(False)]])))
            assert (pl[i, 0] >= 0) == all(one)  # ddave_prob.py:164-165
            if pl[i, 0] < 0:
                assert s[7:].tolist() == [0, 0, w * h, 0] and (z["moves"][i] == -1).all() and z["length"][i] == 0
            elif pl[i, 0] > 0:
                assert s[9] == 0 and s[10] == z["length"][i] == pl[i, 11] > 0 and pl[i, 9] == 1
            else:
                assert s[10] == 0 and z["length"][i] == pl[i, 11]
            # a stage runs only when the one before did not win, and the iterations stay within the power
            assert all(0 <= it <= p for it in pl[i, 1:5])
    assert won == {1, 2, 3, 4} and budget > 20 and emptied > 20 and negative > 5
    assert {("player", 0), ("player", 2), ("exit", 2), ("key", 0), ("regions", 2)} <= pre
    z = _load(7, 11, 5000)
    names = list(z["names"])
    assert z["stats"][names.index("player-on-floor"), 1] == 0 and z["stats"][names.index("player-over-nothing"), 1] == 6
    assert z["stats"][:, 9].min() < -10  # (the heuristic pays 5 per collected diamond)
    # the lure: every A* spends its whole budget on the diamond trail, the BFS wins in three moves
    z = _load(16, 32, 50)
    i = list(z["names"]).index("diamond-lure")
    assert z["play"][i, :5].tolist()[:4] == [4, 50, 50, 50] and z["moves"][i, :3].tolist() == [1, 1, 1] and z["length"][i] == 3
    assert _load(1, 3, 1)["play"][:, 1].max() == 1  # power 1: one iteration per stage


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_rules_equal_fixtures(path):
    z = np.load(path)
    power, cap = int(z["power"]), z["moves"].shape[1]
    for i, m in enumerate(z["grids"]):
        stages = []
        stats, moves, length, play = R.outputs(m, power, cap, key_check={}, stages=stages)  # (both visited keys agree)
        assert stats == z["stats"][i].tolist() and moves == z["moves"][i].tolist() and length == z["length"][i], i
        assert play == z["play"][i].tolist(), i
        assert stages == [s for s in z["stage_node"][i].tolist() if s[2] >= 0], i
        assert not R.has_error(m)
    for a, b, rb, ov, rbc, ovc in zip(z["rew_new"], z["rew_old"], z["rew_bits"], z["over"], z["rew_bits_custom"], z["over_custom"]):
        assert _bits([R.reward(a, b)])[0] == rb and R.episode_over(a) == ov
        weights = dict(zip(R.REWARD_ORDER, z["custom_weights"].tolist()))
        md, ms, tj, ts = (int(v) for v in z["custom_params"])
        assert _bits([R.reward(a, b, weights, md, ms)])[0] == rbc and R.episode_over(a, tj, ts) == ovc


def test_wrong_rules_fail_some_fixture():
    """on two small sets: each wrong rule of ddave_rules.WRONG_RULES changes what some recorded level says"""
    fails = dict.fromkeys(R.WRONG_RULES, 0)
    for h, w, p in ((5, 13, 500), (3, 4, 50)):
        z = _load(h, w, p)
        for i, m in enumerate(z["grids"]):
            if z["play"][i, 0] < 0:
                continue
            for rule in R.WRONG_RULES:
                stages = []
                out = R.outputs(m, p, z["moves"].shape[1], wrong=rule, stages=stages)
                right = (z["stats"][i].tolist(), z["moves"][i].tolist(), z["length"][i], z["play"][i].tolist())
                fails[rule] += out != right or stages != [s for s in z["stage_node"][i].tolist() if s[2] >= 0]
    assert all(fails.values()), fails


def test_rules_on_hand_made_maps():
    # an id above 6 reads as solid and is an error
    m = np.array([[2, 7, 0], [0, 255, 0]], np.uint8)
    assert R.has_error(m) and R.get_stats(m, 5) == R.get_stats(np.array([[2, 1, 0], [0, 1, 0]]), 5)
    # dist-floor: dy - 1 of the first solid below, H - 1 without one, summed over the players; no border
    m = np.array([[2, 2, 0], [0, 0, 0], [1, 0, 0], [0, 0, 2]], np.uint8)
    assert R.dist_floor(m) == 1 + 3 + 3
    # spikes separate regions; solids too
    assert R.num_regions(np.array([[0, 6, 0], [0, 6, 0]])) == 2 and R.num_regions(np.array([[0, 6, 0], [0, 0, 0]])) == 1
    # player, key, door in a row: two moves to the right
    stats, moves, length, play = R.outputs(np.array([[2, 5, 3]]), 50, 4)
    assert stats == [1, 0, 1, 0, 1, 0, 1, 0, 0, 0, 2] and moves == [2, 2, -1, -1] and length == 2
    assert play == [1, 3, 0, 0, 0, 3, 1, 0, 1, 1, 0, 2]  # the root, the step onto the key, the step onto the door
    # the door before the key: the heuristic counts the bordered sizes, (3 + 2) + (1 + 2), while the key lies on the map
    stats, _, _, play = R.outputs(np.array([[2, 3, 5]]), 1, 0)
    assert play[:5] == [0, 1, 1, 1, 1] and stats[9] == 2 + (5 + 3)
    # a diamond is worth 5: dist-win goes negative where nothing else can be done
    stats = R.get_stats(np.array([[4, 2, 1, 5, 3]]), 50)
    assert stats[3] == 1 and stats[6] == 2 and stats[9] == 5  # two regions: not played
    stats, _, _, play = R.outputs(np.array([[4, 2, 0, 0, 0], [1, 1, 1, 5, 3]]), 50, 0)
    assert play[0] > 0 and stats[8] in (0, 1)
    # more than 64 diamonds: not searched, status 5, no error
    m = np.full((8, 11), 4, np.uint8)
    m[7], m[6, :3] = 1, (2, 5, 3)
    stats, _, length, play = R.outputs(m, 50, 0)
    assert stats == [1, 0, 1, 74, 1, 0, 1, 0, 0, 88, 0] and play == [5] + [0] * 9 + [74, 0] and length == 0 and not R.has_error(m)


def test_reward_of_the_rules_on_hand_computed_cases():
    inf = math.inf
    assert R.range_reward(3, 1, inf, inf) == 2 and R.range_reward(1, 3, -inf, -inf) == 2  # more jumps, less dist-win
    assert R.range_reward(5, 2, -inf, 3) == -2 and R.range_reward(2, 3, -inf, 3) == 0  # diamonds above the maximum cost
    assert R.range_reward(12, 7, 10, inf) == 3 and R.range_reward(11, 15, 10, inf) == 0  # spikes up to the minimum pay
    assert R.range_reward(2, 0, 1, 1) == -2 and R.range_reward(1, 0, 1, 1) == 1 and R.range_reward(3, 1, 1, 1) == -2
    old = [1, 0, 1, 0, 1, 10, 1, 0, 0, 77, 0]
    assert R.reward(old, old) == 0
    new = [1, 0, 1, 0, 1, 10, 1, 3, 0, 0, 22]  # solved: three jumps, dist-win 77 -> 0, sol-length 22
    assert R.reward(new, old) == 3 * 3 + 77 * 0.1 + 22 and R.episode_over(new) and not R.episode_over(old)
    assert not R.episode_over([1, 0, 1, 0, 1, 10, 1, 2, 0, 0, 22]) and not R.episode_over([1, 0, 1, 0, 1, 10, 1, 3, 0, 0, 19])
    assert R.reward(new, old, {"dist-win": 0.3}) == 9 + 77 * 0.3 + 22


def test_spec_tables():
    spec = ddave.ddave_spec((7, 11))
    assert spec.name == "ddave" and spec.tile_types == R.TILES == ddave.DDAVE_TILES and spec.n_tiles == 7
    assert spec.stat_keys == R.STAT_KEYS == ddave.DDAVE_STAT_KEYS and spec.default_weights == R.WEIGHTS == spec.problem_weights
    assert tuple(ddave.DDAVE_MOVES) == R.DIRECTIONS and tuple(ddave.DDAVE_REWARD_ORDER) == R.REWARD_ORDER
    cfg = ddave.ddave_config((5, 13), 123, {"dist-win": 0.25}, 4, 5, 6, 7)
    assert (cfg.h, cfg.w, cfg.solver_power, cfg.max_diamonds, cfg.min_spikes, cfg.target_jumps, cfg.target_solution) == \
        (5, 13, 123, 4, 5, 6, 7)
    assert list(cfg.weight) == [3, 2, 3, 1, 1, 3, 5, 3, 0.25, 1]
    with pytest.raises(ValueError):
        ddave.ddave_config(weights={"col-diamonds": 1})


def test_header_units_symbols_and_config():
    _lib.build()
    unit, header = "ddave/pcgrl_k_ddave.hip", "ddave/pcgrl_ddave.h"
    assert unit in _lib.UNITS and header in _lib.HEADERS and "measures/pcgrl_measures_wave.h" in _lib.HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, unit)) and os.path.exists(os.path.join(_lib.CSRC, header))
    assert os.path.exists(_lib.DDAVE_HEADER)
    text = re.sub(r"/\*.*?\*/", "", open(_lib.DDAVE_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(", text))
    assert declared == SYMBOLS == set(_lib.DDAVE_SYMBOLS)
    others = [table for _, table in _lib.ABI if table is not _lib.DDAVE_SYMBOLS]
    assert len(others) == len(_lib.ABI) - 1
    assert not any(declared & set(o) for o in others)
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)  # (exported by the library)
        want = _lib.DDAVE_SYMBOLS[name]
        assert fn.argtypes == want[1] and fn.restype == want[0], name
    for name, params in re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        assert len(params.split(",")) == len(_lib.DDAVE_SYMBOLS[name][1]), name
    # the measures and the diversity take the microstructure argument lists
    for a in ("measures_for_grids", "diversity_scratch_bytes", "diversity_for_grids"):
        assert _lib.DDAVE_SYMBOLS["pcgrl_ddave_" + a] == _lib.MICROSTRUCTURE_SYMBOLS["pcgrl_microstructure_" + a]
    assert C.sizeof(_lib.PcgrlDdaveConfig) == 7 * 4 + 4 + 10 * 8 and _lib.PCGRL_DDAVE_STATS == 11
    m = re.search(r"typedef struct pcgrl_ddave_config \{(.*?)\} pcgrl_ddave_config;", text, flags=re.S)
    fields = re.findall(r"\b([a-z_]+)\s*(?:\[[A-Z_]+\])?\s*[,;]", m.group(1))
    assert fields == [f[0] for f in _lib.PcgrlDdaveConfig._fields_]
    # the kernel is plain HIP C++ that instantiates the shared wave body
    src = open(os.path.join(_lib.CSRC, header)).read()
    assert "asm" not in src.replace("namespace", "")
    assert "meas_wave_map<DD_MEAS_TILES, DD_MEAS_PLANES, DD_MAX_CELLS>" in src
    assert "DD_MEAS_TILES = 7, DD_MEAS_PLANES = 3" in src and "DD_MAX_CELLS = DD_MAX_H * DD_MAX_W" in src
    # the play-through's common parts are written once (playthrough/pcgrl_playthrough.h): one heappop among the four headers
    shared = "playthrough/pcgrl_playthrough.h"
    assert shared in _lib.HEADERS and os.path.exists(os.path.join(_lib.CSRC, shared))
    heads = (shared, "ddave/pcgrl_ddave.h", "mdungeon/pcgrl_mdungeon.h", "smb/pcgrl_smb.h")
    assert [h for h in heads if re.search(r"\w+_heap_pop\(", open(os.path.join(_lib.CSRC, h)).read())] == [shared]
    assert b"0.7.0" in L.pcgrl_version()


def test_workspace_bytes():
    L = _lib.lib()
    ws = L.pcgrl_ddave_workspace_bytes

    def per_level(power):
        cap = 16
        while cap < 2 * power:
            cap *= 2
        nodes = 4 * power + 1
        return nodes * 16 + cap * 12 + (nodes * 4 + 15) // 16 * 16

    assert ws(1, 7, 11, 5000) == per_level(5000) == 596640 and ws(4096, 7, 11, 5000) == 4096 * 596640
    assert ws(3, 1, 1, 1) == 3 * (5 * 16 + 16 * 12 + 32) and ws(1, 16, 32, 16000) == per_level(16000)
    for power in (1, 2, 7, 8, 9, 50, 500, 8192, 8193):
        assert ws(2, 3, 4, power) == 2 * per_level(power) and per_level(power) % 16 == 0
    for args in ((0, 7, 11, 50), (-1, 7, 11, 50)):
        assert ws(*args) < 0 and b"pcgrl_ddave_workspace_bytes: n must be at least 1" in L.pcgrl_last_error()
    for args in ((1, 0, 11, 50), (1, 17, 11, 50), (1, 7, 0, 50), (1, 7, 33, 50)):
        assert ws(*args) < 0 and b"pcgrl_ddave_workspace_bytes: maps of 1..16 rows and 1..32 columns" in L.pcgrl_last_error()
    for args in ((1, 7, 11, 0), (1, 7, 11, 16001), (1, 7, 11, -5)):
        assert ws(*args) < 0 and b"pcgrl_ddave_workspace_bytes: solver_power must be in [1, 16000]" in L.pcgrl_last_error()
    assert "596 640" in ddave.DDaveEvaluator.__doc__  # the class docstring states the figure at the stock power


def test_abi_argument_checks_need_no_device():
    L = _lib.lib()
    # pointers that are never dereferenced: every call below is refused before any HIP call
    grids, stats, wsp = 0x1000, 0x3000, 0x10000
    EINVAL, EUNSUPPORTED = 1, 2
    who = b"pcgrl_ddave_evaluate:"
    big = 1 << 40

    def call(cfg, n=2, g=grids, ws=wsp, ws_bytes=big, cap=8, st=stats):
        return L.pcgrl_ddave_evaluate(C.byref(cfg) if cfg is not None else None, n, g, ws, ws_bytes, cap, st, None, None, None,
                                      None, None)

    ok = ddave.ddave_config((7, 11), 50)
    for kw in (dict(cfg=None), dict(cfg=ok, g=None), dict(cfg=ok, st=None), dict(cfg=ok, n=0), dict(cfg=ok, n=-3)):
        assert call(**kw) == EINVAL and who in L.pcgrl_last_error(), kw
    assert call(ok, cap=-1) == EINVAL and who + b" move_cap must not be negative" in L.pcgrl_last_error()
    need = L.pcgrl_ddave_workspace_bytes(2, 7, 11, 50)
    for kw in (dict(ws=None), dict(ws=wsp + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(ok, **kw) == EINVAL and who + b" the workspace is null, not 16-byte aligned or smaller" in L.pcgrl_last_error()
    for shape in ((0, 12), (17, 12), (8, 0), (8, 33), (-1, 4)):
        assert call(ddave.ddave_config(shape, 50)) == EUNSUPPORTED, shape
        assert who in L.pcgrl_last_error() and b"1..16 rows and 1..32 columns" in L.pcgrl_last_error()
    for power in (0, 16001, -1):
        assert call(ddave.ddave_config((7, 11), power)) == EUNSUPPORTED
        assert who + b" solver_power must be in [1, 16000]" in L.pcgrl_last_error()

    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    p += 8 - p % 8
    meas, div = L.pcgrl_ddave_measures_for_grids, L.pcgrl_ddave_diversity_for_grids
    scratch = L.pcgrl_ddave_diversity_scratch_bytes
    for args in ((7, 11, 1, None, p, p, None, None, None, None), (7, 11, 1, p, None, p, None, None, None, None),
                 (7, 11, 1, p, p, None, None, None, None, None), (7, 11, 1, p, p, p, None, p, None, None),
                 (7, 11, -1, p, p, p, None, None, None, None)):
        assert meas(*args) == EINVAL and b"pcgrl_ddave_measures_for_grids:" in L.pcgrl_last_error()
    rest = (None,) * 6
    for args in ((7, 11, 8, None, 4, p, p), (7, 11, 8, p, 4, None, p), (7, 11, 8, p, 4, p, None), (7, 11, 8, p, 4, p + 4, p),
                 (7, 11, -8, p, 4, p, p)):
        assert div(*args, *rest) == EINVAL and b"pcgrl_ddave_diversity_for_grids:" in L.pcgrl_last_error()
    for h, w in ((0, 12), (17, 12), (8, 0), (8, 33)):
        assert meas(h, w, 1, p, p, p, None, None, None, None) == EUNSUPPORTED
        assert b"pcgrl_ddave_measures_for_grids: maps of 1..16 rows and 1..32 columns" in L.pcgrl_last_error()
        assert div(h, w, 8, p, 4, p, p, *rest) == EUNSUPPORTED
        assert b"pcgrl_ddave_diversity_for_grids: maps of 1..16 rows and 1..32 columns" in L.pcgrl_last_error()
        assert scratch(h, w, 8) == 0
    for group in (1, 3, 0, -2):
        assert div(7, 11, 8, p, group, p, p, *rest) == EINVAL
        assert b"group must be at least 2 and divide the number of maps" in L.pcgrl_last_error()
    # no maps: a no-op
    assert meas(7, 11, 0, None, None, None, None, None, None, None) == 0
    assert div(7, 11, 0, None, 4, None, None, None, None, None, None, None) == 0
    assert scratch(7, 11, 0) == 0 and scratch(7, 11, -3) == 0
    # 8 * (3 * ceil(h * w / 64) + 1) per map: three planes
    assert scratch(1, 1, 3) == 3 * 4 * 8 and scratch(16, 32, 4096) == 4096 * 25 * 8 and scratch(7, 11, 1) == 7 * 8

    for shape, power in (((0, 12), 50), ((17, 12), 50), ((8, 33), 50), ((7, 11), 0), ((7, 11), 16001)):
        with pytest.raises(NotImplementedError):
            ddave.DDaveEvaluator(shape, device="cuda:0", solver_power=power)
    with pytest.raises(ValueError):
        ddave.DDaveEvaluator((7, 11), device="cpu", solver_power=5, max_levels=1)  # no CPU fallback
    with pytest.raises(ValueError):
        ddave.DDaveEvaluator((7, 11, 2))
    with pytest.raises(ValueError):
        ddave.DDaveEvaluator((7, 11), max_levels=0)


def test_python_surface_is_in_place():
    import control_pcgrl_amd
    from control_pcgrl_amd import DDAVE_BC_NAMES, DDaveEvaluator
    from control_pcgrl_amd.measures import MeasuresMixin
    E = DDaveEvaluator
    assert issubclass(E, MeasuresMixin) and E is ddave.DDaveEvaluator
    assert control_pcgrl_amd.ddave_spec is ddave.ddave_spec
    sig = inspect.signature(E.__init__).parameters
    assert list(sig) == ["self", "map_shape", "device", "solver_power", "weights", "max_diamonds", "min_spikes", "target_jumps",
                         "target_solution", "max_levels"]
    assert [sig[k].default for k in list(sig)[1:]] == [(7, 11), "cuda:0", 5000, None, 3, 10, 2, 20, 4096]
    assert list(inspect.signature(E.evaluate).parameters) == ["self", "grids", "move_cap"]
    assert inspect.signature(E.evaluate).parameters["move_cap"].default == 0
    assert list(inspect.signature(E.reward).parameters) == ["self", "new_stats", "old_stats"]
    assert list(inspect.signature(E.episode_over).parameters) == ["self", "stats"]
    assert list(inspect.signature(E.measures).parameters) == ["self", "grids", "entropy"]
    assert inspect.signature(E.measures).parameters["entropy"].default is True
    sig = inspect.signature(E.diversity).parameters
    assert list(sig) == ["self", "grids", "group", "pairwise"] and sig["group"].default is None and sig["pairwise"].default is False
    assert list(inspect.signature(E.behaviour).parameters) == ["self", "grids", "names"]
    assert list(inspect.signature(E.check_errors).parameters) == ["self"] and list(inspect.signature(E.close).parameters) == ["self"]
    assert hasattr(E, "__enter__") and hasattr(E, "__exit__")
    assert DDAVE_BC_NAMES is ddave.DDAVE_BC_NAMES
    assert tuple(DDAVE_BC_NAMES) == tuple(R.STAT_KEYS) + ("emptiness", "entropy", "symmetry", "symmetry-horizontal",
                                                          "symmetry-vertical", "co-occurance", "NONE")
    assert tuple(DDAVE_BC_NAMES[11:17]) == tuple(mn.BC_NAMES) == tuple(ddave.DDAVE_MEASURE_NAMES)
    assert ddave.DDAVE_TILES == R.TILES and len(ddave.DDAVE_PLAY_KEYS) == R.PLAY_FIELDS == 12
    assert "stepping Dangerous Dave environments is not built" in ddave.__doc__


def test_ddave_stays_outside_the_engine():
    import control_pcgrl_amd
    assert "ddave" not in problems.PROBLEMS
    with pytest.raises(ValueError):
        problems.problem_spec("ddave", (7, 11))
    with pytest.raises(ValueError):
        build_config("ddave", "narrow", (7, 11))
    assert control_pcgrl_amd.__version__ == "0.7.0" and b"0.7.0" in _lib.lib().pcgrl_version()
