"""MiniDungeon levels, the parts that need no GPU: the plain-Python rules (tests/mdungeon_rules.py) against the fixtures recorded
from the reference (tests/golden/mdungeon, tools/gen_golden_mdungeon.py), the cases the fixtures hold, the restated reward on
hand-computed cases, the header, the symbols and the config struct, the argument checks of the C ABI
(include/pcgrl_amd_mdungeon.h: made before any HIP call, so they answer without a device), the workspace sizes, the Python
surface, and what stays outside the engine."""
import ctypes as C
import glob
import inspect
import math
import os
import re

import numpy as np
import pytest

import mdungeon_levels as ML
import mdungeon_rules as R
import measures_numpy as mn
from conftest import GOLDEN
from control_pcgrl_amd import _lib, mdungeon, problems
from control_pcgrl_amd.vec_env import build_config

DIR = os.path.join(GOLDEN, "mdungeon")
FILES = sorted(glob.glob(os.path.join(DIR, "md_*.npz")))
SMALL = ((1, 1), (1, 2), (1, 3), (2, 3), (3, 4), (5, 13), (16, 32))
SETS = [(11, 7, 5000)] + [(h, w, p) for h, w in SMALL for p in (1, 2, 50, 500)]
MEAS_SHAPES = [(1, 1), (1, 32), (16, 1), (5, 2), (5, 13), (11, 7), (16, 32)]
SYMBOLS = {"pcgrl_mdungeon_workspace_bytes", "pcgrl_mdungeon_evaluate", "pcgrl_mdungeon_measures_for_grids",
           "pcgrl_mdungeon_diversity_scratch_bytes", "pcgrl_mdungeon_diversity_for_grids"}


def _bits(values):
    return np.asarray([float(v) for v in values], np.float64).view(np.uint64)


def _load(h, w, power):
    return np.load(os.path.join(DIR, f"md_{h}x{w}_p{power}.npz"))


def _items(grids):
    return (grids >= ML.POTION).reshape(len(grids), -1).sum(1)


def test_fixture_set_is_complete():
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(DIR, "*.npz")))
    assert names == sorted([f"md_{h}x{w}_p{p}.npz" for h, w, p in SETS] + [f"meas_{h}x{w}.npz" for h, w in MEAS_SHAPES])
    assert max(os.path.getsize(os.path.join(DIR, f)) for f in names) <= 100 * 1024
    for h, w, p in SETS:
        z = _load(h, w, p)  # (allow_pickle is off: arrays only)
        n = len(z["grids"])
        assert z["grids"].dtype == np.uint8 and z["grids"].shape[1:] == (h, w) and z["grids"].max() <= 7 and int(z["power"]) == p
        assert list(z["stat_keys"]) == R.STAT_KEYS and z["stats"].shape == (n, 11) and z["stats"].dtype == np.int32
        assert z["stage_iters"].shape == z["stage_won"].shape == (n, 4) and z["stage_node"].shape == (n, 4, 3)
        assert z["play"].shape == (n, 12) and z["length"].shape == (n,) and z["moves"].shape[0] == n and len(z["names"]) == n
        assert z["moves"].shape[1] == max(1, z["length"].max())  # every move of every level is recorded
        m = len(z["rew_new"])
        assert m >= 96 and z["rew_old"].shape == (m, 11) and z["rew_bits"].shape == z["rew_bits_custom"].shape == (m,)
        assert z["over"].shape == z["over_custom"].shape == (m,) and z["custom_weights"].shape == (9,)
        assert z["custom_params"].shape == (4,) and z["custom_target_col_enemies"].shape == ()
        assert _items(z["grids"]).max() <= R.MAX_ITEMS
    assert len(_load(11, 7, 5000)["grids"]) >= 200


def test_fixtures_show_the_cases():
    won, budget, emptied, negative, pre = set(), 0, 0, 0, set()
    for h, w, p in SETS:
        z = _load(h, w, p)
        st, pl = z["stats"], z["play"]
        won |= set(pl[:, 0][pl[:, 0] > 0].tolist())
        budget += int(((pl[:, 0] == 0) & (pl[:, 4] == p)).sum())
        emptied += int(((pl[:, 0] == 0) & (pl[:, 4] < p)).sum())
        negative += int((st[:, 9] < 0).sum())
        assert (st[:, 4] == (z["grids"] >= ML.GOBLIN).reshape(len(st), -1).sum(1)).all()  # goblins and ogres together
        for i, s in enumerate(st):
            one = [s[j] == 1 for j in (0, 1, 5)]
            if sum(one) == 2:
                pre.add((("player", "exit", "regions")[one.index(False)], int(s[(0, 1, 5)[one.index(False)]])))
            assert (pl[i, 0] >= 0) == all(one)  # mdungeon_prob.py:166
            if pl[i, 0] < 0:
                assert s[6:].tolist() == [0, 0, 0, w * h, 0] and (z["moves"][i] == -1).all() and z["length"][i] == 0
                assert pl[i].tolist() == [-1] + [0] * 11
            elif pl[i, 0] > 0:
                assert s[9] == 0 and s[10] == z["length"][i] == pl[i, 11] > 0 and pl[i, 7] > 0
            else:
                assert s[10] == 0 and z["length"][i] == pl[i, 11]
            if pl[i, 0] >= 0:
                assert s[6:9].tolist() == pl[i, 8:11].tolist() and 0 <= pl[i, 7] <= 5
            assert all(0 <= it <= p for it in pl[i, 1:5])
    assert won == {1, 2, 3, 4} and budget > 20 and emptied > 20 and negative >= 2
    assert {("player", 0), ("player", 2), ("exit", 0), ("exit", 2), ("regions", 2)} <= pre
    z = _load(11, 7, 5000)
    names = list(z["names"])
    # three ogres in a corridor: the player dies on the third, every route is lost, the open list empties
    i = names.index("three-ogres")
    assert z["play"][i, 0] == 0 and (z["play"][i, 1:5] < 5000).all() and z["stats"][i, 10] == 0
    # a potion at full health is consumed and counted; goblin then potion ends at 5, clamped
    i = names.index("potion-at-full-health")
    assert z["play"][i, [0, 7, 8]].tolist() == [1, 5, 1] and z["stats"][i, 6] == 1 and z["length"][i] == 3
    i = names.index("goblin-then-potion")
    assert z["play"][i, [0, 7, 8, 10]].tolist() == [1, 5, 1, 1] and z["length"][i] == 4
    # the guarded exits take thousands of iterations (a win needs retreats to the potions between the ogres), and some spend
    # all four budgets
    guarded = [i for i, k in enumerate(names) if k.startswith("guarded_exit")]
    assert len(guarded) == 4 and (z["play"][guarded, 1:5].sum(1) > 5000).all()
    assert (z["play"][guarded, :5] == [0, 5000, 5000, 5000, 5000]).all(1).any()
    assert z["stats"][:, 9].min() < -10  # (the heuristic pays 4 per collected treasure)
    # the lure: every A* spends its whole budget on the treasure trail, the BFS wins in two moves
    z = _load(16, 32, 50)
    i = list(z["names"]).index("treasure-lure")
    assert z["play"][i, :4].tolist() == [4, 50, 50, 50]
    assert z["moves"][i, :2].tolist() == [0, 0] and z["length"][i] == 2
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
    weights = dict(zip(R.REWARD_ORDER, z["custom_weights"].tolist()))
    me, mp, mt, ts = (int(v) for v in z["custom_params"])
    tc = float(z["custom_target_col_enemies"])
    for a, b, rb, ov, rbc, ovc in zip(z["rew_new"], z["rew_old"], z["rew_bits"], z["over"], z["rew_bits_custom"], z["over_custom"]):
        assert _bits([R.reward(a, b)])[0] == rb and R.episode_over(a) == ov
        assert _bits([R.reward(a, b, weights, me, mp, mt)])[0] == rbc and R.episode_over(a, tc, ts) == ovc


def test_wrong_rules_fail_some_fixture():
    """on two small sets: each wrong rule of mdungeon_rules.WRONG_RULES changes what some recorded level says"""
    fails = dict.fromkeys(R.WRONG_RULES, 0)
    assert len(R.WRONG_RULES) >= 5
    for h, w, p in ((5, 13, 500), (5, 13, 50), (3, 4, 50)):
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
    # an id above 7 reads as solid and is an error
    m = np.array([[2, 8, 0], [0, 255, 0]], np.uint8)
    assert R.has_error(m) and R.get_stats(m, 5) == R.get_stats(np.array([[2, 1, 0], [0, 1, 0]]), 5)
    # only solids separate regions; enemies and items do not
    assert R.num_regions(np.array([[0, 1, 0], [0, 1, 0]])) == 2 and R.num_regions(np.array([[0, 7, 0], [4, 1, 6]])) == 1
    # player, a free cell, door in a row: two moves to the right.  Pops: the root (heuristic 2), the child at heuristic 1, the door
    stats, moves, length, play = R.outputs(np.array([[2, 0, 3]]), 50, 4)
    assert stats == [1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 2] and moves == [1, 1, -1, -1] and length == 2
    assert play == [1, 3, 0, 0, 0, 3, 1, 5, 0, 0, 0, 2]
    # power 1: each stage pops the root and returns it; dist-win is its heuristic
    stats, _, _, play = R.outputs(np.array([[2, 0, 3]]), 1, 0)
    assert play == [0, 1, 1, 1, 1, 1, 1, 5, 0, 0, 0, 0] and stats[9] == 2 and stats[10] == 0
    # a goblin on the way costs 1 health, an ogre 2; both are counted as enemies
    stats, moves, _, play = R.outputs(np.array([[2, 6, 7, 3]]), 50, 3)
    assert stats == [1, 1, 0, 0, 2, 1, 0, 0, 2, 0, 3] and moves == [1, 1, 1] and play[7:11] == [2, 0, 0, 2]
    # three ogres: 5 -> 3 -> 1 -> 0 (clamped), lost before the door; no stage wins and every open list empties.  The best
    # node is the root: heuristic 4, against 3 + 8 after one ogre and 2 + 16 after two
    stats, moves, length, play = R.outputs(np.array([[2, 7, 7, 7, 3]]), 50, 2)
    assert play[0] == 0 and all(it < 50 for it in play[1:5]) and stats[6:] == [0, 0, 0, 4, 0] and length == 0 and moves == [-1, -1]
    # a treasure is worth 4: with the door out of reach of the budget, dist-win goes negative.  One iteration expands the root,
    # two more are the root's children; the BFS pops left (a wall: the root's key again) and then right (the treasure: 3 - 4)
    stats, _, _, play = R.outputs(np.array([[2, 5, 0, 0, 3]]), 3, 0)
    assert play[:5] == [0, 3, 3, 3, 3] and stats[9] == -1 and stats[7] == 1
    # potion then goblin ends at health 4, goblin then potion at 5: the same items are gone, the keys differ
    lv = R.Level(R.clean(np.array([[2, 4, 6, 0, 3], [0, 0, 0, 0, 0]])))
    root = R.Node()
    root.x, root.y, root.health, root.potions, root.treasures, root.enemies = 1, 1, 5, 0, 0, 0
    root.left, root.depth, root.parent, root.action = frozenset(lv.potions + lv.enemies), 0, None, None
    a = R.child(lv, R.child(lv, root, 1), 1)  # right onto the potion (health stays 5), right onto the goblin
    b = root
    for act in (3, 1, 1, 2, 0):  # down, right, right, up onto the goblin, left onto the potion
        b = R.child(lv, b, act)
    assert (a.health, b.health) == (4, 5) and a.left == b.left == frozenset() and (a.potions, a.enemies) == (1, 1)
    assert R.string_key(lv, a) != R.string_key(lv, R.child(lv, b, 1))  # the same cell and items, another health
    # State.getKey's trimming (engine.py:277, :280, :283): an empty list's [:-1] eats the separator before it, so with every
    # list empty all three collapse, and the empty treasure list between potions and enemies leaves one "|", not two
    assert R.string_key(lv, a) == "3,1,4|5,1"
    assert R.string_key(lv, root) == "1,1,5|5,1|2,1|3,1"
    # more than 64 items: not searched, status 5, pre-search statistics, no error
    m = np.full((8, 11), 5, np.uint8)
    m[7], m[6, :3] = 1, (2, 0, 3)
    stats, _, length, play = R.outputs(m, 50, 0)
    assert stats == [1, 1, 0, 74, 0, 1, 0, 0, 0, 88, 0] and play == [5] + [0] * 11 and length == 0 and not R.has_error(m)


def test_reward_of_the_rules_on_hand_computed_cases():
    inf = math.inf
    assert R.range_reward(3, 1, inf, inf) == 2 and R.range_reward(1, 3, -inf, -inf) == 2  # more col-enemies, less dist-win
    assert R.range_reward(5, 2, -inf, 3) == -2 and R.range_reward(2, 3, -inf, 3) == 0  # treasures above the maximum cost
    assert R.range_reward(8, 3, 1, 6) == -2 and R.range_reward(0, 2, 1, 6) == -1 and R.range_reward(4, 2, 1, 6) == 0
    assert R.range_reward(2, 0, 1, 1) == -2 and R.range_reward(1, 0, 1, 1) == 1 and R.range_reward(3, 1, 1, 1) == -2
    old = [1, 1, 1, 1, 4, 1, 0, 0, 0, 77, 0]
    assert R.reward(old, old) == 0
    new = [1, 1, 1, 1, 4, 1, 1, 0, 3, 0, 22]  # solved: three enemies met, dist-win 77 -> 0, sol-length 22
    assert R.reward(new, old) == 3 * 2 + 77 * 0.1 + 22 and R.episode_over(new) and not R.episode_over(old)
    assert not R.episode_over([1, 1, 1, 1, 4, 1, 1, 0, 2, 0, 22])  # 2 / 4 is not above 0.5
    assert not R.episode_over([1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 22]) and not R.episode_over([1, 1, 1, 1, 4, 1, 1, 0, 3, 0, 19])
    assert R.episode_over([1, 1, 1, 1, 4, 1, 1, 0, 2, 0, 22], 0.25) and R.episode_over([1, 1, 1, 1, 4, 1, 1, 0, 3, 0, 19], 0.5, 19)
    assert R.reward(new, old, {"dist-win": 0.3}) == 6 + 77 * 0.3 + 22
    assert R.reward([1, 1, 4, 5, 9, 1, 0, 0, 0, 0, 0], [1, 1, 2, 3, 6, 1, 0, 0, 0, 0, 0]) == -3 * 2 - 2 - 2


def test_spec_tables():
    spec = mdungeon.mdungeon_spec((11, 7))
    assert spec.name == "mdungeon" and spec.tile_types == R.TILES == mdungeon.MDUNGEON_TILES and spec.n_tiles == 8
    assert spec.stat_keys == R.STAT_KEYS == mdungeon.MDUNGEON_STAT_KEYS
    assert spec.default_weights == R.WEIGHTS == spec.problem_weights
    assert tuple(mdungeon.MDUNGEON_MOVES) == R.DIRECTIONS and tuple(mdungeon.MDUNGEON_REWARD_ORDER) == R.REWARD_ORDER
    cfg = mdungeon.mdungeon_config((5, 13), 123, {"dist-win": 0.25}, 4, 5, 6, 0.75, 7)
    assert (cfg.h, cfg.w, cfg.solver_power, cfg.max_enemies, cfg.max_potions, cfg.max_treasures, cfg.target_solution,
            cfg.target_col_enemies) == (5, 13, 123, 4, 5, 6, 7, 0.75)
    assert list(cfg.weight) == [3, 3, 2, 1, 1, 5, 2, 0.25, 1]
    with pytest.raises(ValueError):
        mdungeon.mdungeon_config(weights={"col-potions": 1})


def test_header_units_symbols_and_config():
    _lib.build()
    unit, header = "mdungeon/pcgrl_k_mdungeon.hip", "mdungeon/pcgrl_mdungeon.h"
    assert unit in _lib.UNITS and header in _lib.HEADERS and "measures/pcgrl_measures_wave.h" in _lib.HEADERS
    assert os.path.exists(os.path.join(_lib.CSRC, unit)) and os.path.exists(os.path.join(_lib.CSRC, header))
    assert os.path.exists(_lib.MDUNGEON_HEADER)
    text = re.sub(r"/\*.*?\*/", "", open(_lib.MDUNGEON_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(", text))
    assert declared == SYMBOLS == set(_lib.MDUNGEON_SYMBOLS)
    others = [table for _, table in _lib.ABI if table is not _lib.MDUNGEON_SYMBOLS]
    assert len(others) == len(_lib.ABI) - 1
    assert not any(declared & set(o) for o in others)
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)  # (exported by the library)
        want = _lib.MDUNGEON_SYMBOLS[name]
        assert fn.argtypes == want[1] and fn.restype == want[0], name
    for name, params in re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        assert len(params.split(",")) == len(_lib.MDUNGEON_SYMBOLS[name][1]), name
    # the measures and the diversity take the microstructure argument lists
    for a in ("measures_for_grids", "diversity_scratch_bytes", "diversity_for_grids"):
        assert _lib.MDUNGEON_SYMBOLS["pcgrl_mdungeon_" + a] == _lib.MICROSTRUCTURE_SYMBOLS["pcgrl_microstructure_" + a]
    assert C.sizeof(_lib.PcgrlMdungeonConfig) == 7 * 4 + 4 + 8 + 9 * 8 and _lib.PCGRL_MDUNGEON_STATS == 11
    assert _lib.PCGRL_MDUNGEON_WEIGHTS == 9 == len(R.REWARD_ORDER) and _lib.PCGRL_MDUNGEON_PLAY == 12
    assert _lib.PcgrlMdungeonConfig.target_col_enemies.offset == 32 and _lib.PcgrlMdungeonConfig.weight.offset == 40
    m = re.search(r"typedef struct pcgrl_mdungeon_config \{(.*?)\} pcgrl_mdungeon_config;", text, flags=re.S)
    fields = re.findall(r"\b([a-z_]+)\s*(?:\[[A-Z_]+\])?\s*[,;]", m.group(1))
    assert fields == [f[0] for f in _lib.PcgrlMdungeonConfig._fields_]
    # the kernel is plain HIP C++ that instantiates the shared wave body
    src = open(os.path.join(_lib.CSRC, header)).read()
    assert "asm" not in src.replace("namespace", "")
    assert "meas_wave_map<MD_MEAS_TILES, MD_MEAS_PLANES, MD_MAX_CELLS>" in src
    assert "MD_MEAS_TILES = 8, MD_MEAS_PLANES = 3" in src and "MD_MAX_CELLS = MD_MAX_H * MD_MAX_W" in src
    # the open list's integer image: the bias and the 16-bit bound follow from the item limit
    assert "MD_F_BIAS = 2 * 4 * MD_MAX_ITEMS" in src and "MD_MAX_ITEMS = 64" in src
    assert 2 * (33 + 17 + 20) + 2 * 16000 + 2 * 4 * 64 < 1 << 16
    # the play-through's common parts are written once (playthrough/pcgrl_playthrough.h): one heappop among the four headers
    shared = "playthrough/pcgrl_playthrough.h"
    assert shared in _lib.HEADERS and os.path.exists(os.path.join(_lib.CSRC, shared))
    heads = (shared, "ddave/pcgrl_ddave.h", "mdungeon/pcgrl_mdungeon.h", "smb/pcgrl_smb.h")
    assert [h for h in heads if re.search(r"\w+_heap_pop\(", open(os.path.join(_lib.CSRC, h)).read())] == [shared]
    assert b"0.7.0" in L.pcgrl_version()


def test_workspace_bytes():
    L = _lib.lib()
    ws = L.pcgrl_mdungeon_workspace_bytes

    def per_level(power):
        cap = 16
        while cap < 2 * power:
            cap *= 2
        nodes = 4 * power + 1
        return nodes * 16 + cap * 12 + (nodes * 4 + 15) // 16 * 16

    assert ws(1, 11, 7, 5000) == per_level(5000) == 596640 and ws(4096, 11, 7, 5000) == 4096 * 596640
    assert ws(3, 1, 1, 1) == 3 * (5 * 16 + 16 * 12 + 32) and ws(1, 16, 32, 16000) == per_level(16000)
    for power in (1, 2, 7, 8, 9, 50, 500, 8192, 8193):
        assert ws(2, 3, 4, power) == 2 * per_level(power) and per_level(power) % 16 == 0
    for args in ((0, 11, 7, 50), (-1, 11, 7, 50)):
        assert ws(*args) < 0 and b"pcgrl_mdungeon_workspace_bytes: n must be at least 1" in L.pcgrl_last_error()
    for args in ((1, 0, 11, 50), (1, 17, 11, 50), (1, 7, 0, 50), (1, 7, 33, 50)):
        assert ws(*args) < 0 and b"pcgrl_mdungeon_workspace_bytes: maps of 1..16 rows and 1..32 columns" in L.pcgrl_last_error()
    for args in ((1, 11, 7, 0), (1, 11, 7, 16001), (1, 11, 7, -5)):
        assert ws(*args) < 0 and b"pcgrl_mdungeon_workspace_bytes: solver_power must be in [1, 16000]" in L.pcgrl_last_error()
    assert "596 640" in mdungeon.MDungeonEvaluator.__doc__  # the class docstring states the figure at the stock power


def test_abi_argument_checks_need_no_device():
    L = _lib.lib()
    # pointers that are never dereferenced: every call below is refused before any HIP call
    grids, stats, wsp = 0x1000, 0x3000, 0x10000
    EINVAL, EUNSUPPORTED = 1, 2
    who = b"pcgrl_mdungeon_evaluate:"
    big = 1 << 40

    def call(cfg, n=2, g=grids, ws=wsp, ws_bytes=big, cap=8, st=stats):
        return L.pcgrl_mdungeon_evaluate(C.byref(cfg) if cfg is not None else None, n, g, ws, ws_bytes, cap, st, None, None,
                                         None, None, None)

    ok = mdungeon.mdungeon_config((11, 7), 50)
    for kw in (dict(cfg=None), dict(cfg=ok, g=None), dict(cfg=ok, st=None), dict(cfg=ok, n=0), dict(cfg=ok, n=-3)):
        assert call(**kw) == EINVAL and who in L.pcgrl_last_error(), kw
    assert call(ok, cap=-1) == EINVAL and who + b" move_cap must not be negative" in L.pcgrl_last_error()
    need = L.pcgrl_mdungeon_workspace_bytes(2, 11, 7, 50)
    for kw in (dict(ws=None), dict(ws=wsp + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(ok, **kw) == EINVAL and who + b" the workspace is null, not 16-byte aligned or smaller" in L.pcgrl_last_error()
    for shape in ((0, 12), (17, 12), (8, 0), (8, 33), (-1, 4)):
        assert call(mdungeon.mdungeon_config(shape, 50)) == EUNSUPPORTED, shape
        assert who in L.pcgrl_last_error() and b"1..16 rows and 1..32 columns" in L.pcgrl_last_error()
    for power in (0, 16001, -1):
        assert call(mdungeon.mdungeon_config((11, 7), power)) == EUNSUPPORTED
        assert who + b" solver_power must be in [1, 16000]" in L.pcgrl_last_error()

    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    p += 8 - p % 8
    meas, div = L.pcgrl_mdungeon_measures_for_grids, L.pcgrl_mdungeon_diversity_for_grids
    scratch = L.pcgrl_mdungeon_diversity_scratch_bytes
    for args in ((11, 7, 1, None, p, p, None, None, None, None), (11, 7, 1, p, None, p, None, None, None, None),
                 (11, 7, 1, p, p, None, None, None, None, None), (11, 7, 1, p, p, p, None, p, None, None),
                 (11, 7, -1, p, p, p, None, None, None, None)):
        assert meas(*args) == EINVAL and b"pcgrl_mdungeon_measures_for_grids:" in L.pcgrl_last_error()
    rest = (None,) * 6
    for args in ((11, 7, 8, None, 4, p, p), (11, 7, 8, p, 4, None, p), (11, 7, 8, p, 4, p, None), (11, 7, 8, p, 4, p + 4, p),
                 (11, 7, -8, p, 4, p, p)):
        assert div(*args, *rest) == EINVAL and b"pcgrl_mdungeon_diversity_for_grids:" in L.pcgrl_last_error()
    for h, w in ((0, 12), (17, 12), (8, 0), (8, 33)):
        assert meas(h, w, 1, p, p, p, None, None, None, None) == EUNSUPPORTED
        assert b"pcgrl_mdungeon_measures_for_grids: maps of 1..16 rows and 1..32 columns" in L.pcgrl_last_error()
        assert div(h, w, 8, p, 4, p, p, *rest) == EUNSUPPORTED
        assert b"pcgrl_mdungeon_diversity_for_grids: maps of 1..16 rows and 1..32 columns" in L.pcgrl_last_error()
        assert scratch(h, w, 8) == 0
    for group in (1, 3, 0, -2):
        assert div(11, 7, 8, p, group, p, p, *rest) == EINVAL
        assert b"group must be at least 2 and divide the number of maps" in L.pcgrl_last_error()
    # no maps: a no-op
    assert meas(11, 7, 0, None, None, None, None, None, None, None) == 0
    assert div(11, 7, 0, None, 4, None, None, None, None, None, None, None) == 0
    assert scratch(11, 7, 0) == 0 and scratch(11, 7, -3) == 0
    # 8 * (3 * ceil(h * w / 64) + 1) per map: three planes
    assert scratch(1, 1, 3) == 3 * 4 * 8 and scratch(16, 32, 4096) == 4096 * 25 * 8 and scratch(11, 7, 1) == 7 * 8


def test_python_refusals():
    for shape, power in (((0, 12), 50), ((17, 12), 50), ((8, 33), 50), ((11, 7), 0), ((11, 7), 16001)):
        with pytest.raises(NotImplementedError):
            mdungeon.MDungeonEvaluator(shape, device="cuda:0", solver_power=power)
    with pytest.raises(ValueError):
        mdungeon.MDungeonEvaluator((11, 7), device="cpu", solver_power=5, max_levels=1)  # no CPU fallback
    with pytest.raises(ValueError):
        mdungeon.MDungeonEvaluator((11, 7, 2))
    with pytest.raises(ValueError):
        mdungeon.MDungeonEvaluator((11, 7), max_levels=0)
    with pytest.raises(ValueError):
        mdungeon.MDungeonEvaluator((11, 7), weights={"col-potions": 1})


def test_python_surface_is_in_place():
    import control_pcgrl_amd
    from control_pcgrl_amd import MDUNGEON_BC_NAMES, MDungeonEvaluator
    from control_pcgrl_amd.measures import MeasuresMixin
    E = MDungeonEvaluator
    assert issubclass(E, MeasuresMixin) and E is mdungeon.MDungeonEvaluator
    assert control_pcgrl_amd.mdungeon_spec is mdungeon.mdungeon_spec
    sig = inspect.signature(E.__init__).parameters
    assert list(sig) == ["self", "map_shape", "device", "solver_power", "weights", "max_enemies", "max_potions", "max_treasures",
                         "target_col_enemies", "target_solution", "max_levels"]
    assert [sig[k].default for k in list(sig)[1:]] == [(11, 7), "cuda:0", 5000, None, 6, 2, 3, 0.5, 20, 4096]
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
    assert MDUNGEON_BC_NAMES is mdungeon.MDUNGEON_BC_NAMES
    assert tuple(MDUNGEON_BC_NAMES) == tuple(R.STAT_KEYS) + ("emptiness", "entropy", "symmetry", "symmetry-horizontal",
                                                             "symmetry-vertical", "co-occurance", "NONE")
    assert tuple(MDUNGEON_BC_NAMES[11:17]) == tuple(mn.BC_NAMES) == tuple(mdungeon.MDUNGEON_MEASURE_NAMES)
    assert mdungeon.MDUNGEON_TILES == R.TILES and len(mdungeon.MDUNGEON_PLAY_KEYS) == R.PLAY_FIELDS == 12
    assert mdungeon.MDUNGEON_WEIGHTS == R.WEIGHTS and mdungeon.MAX_ITEMS == R.MAX_ITEMS == ML.MAX_ITEMS == 64
    assert "stepping MiniDungeon environments is not built" in mdungeon.__doc__


def test_generators_cap_the_items():
    rng = np.random.default_rng(5)
    maps = ML.mixed(rng, 16, 32, 64)
    assert maps.dtype == np.uint8 and maps.max() <= 7 and _items(maps).max() <= 64 and (_items(maps) == 64).any()
    m = np.full((16, 32), ML.TREASURE, np.uint8)
    capped = ML.cap_items(m.copy())
    assert (capped.ravel()[:64] == ML.TREASURE).all() and (capped.ravel()[64:] == ML.EMPTY).all()  # row-major: the surplus empties
    for gen in ML.GENERATORS:
        assert gen(rng, 1, 1).shape == (1, 1) and gen(rng, 1, 2).shape == (1, 2)


def test_mdungeon_stays_outside_the_engine():
    import control_pcgrl_amd
    assert "mdungeon" not in problems.PROBLEMS
    with pytest.raises(ValueError):
        problems.problem_spec("mdungeon", (11, 7))
    with pytest.raises(ValueError):
        build_config("mdungeon", "narrow", (11, 7))
    assert control_pcgrl_amd.__version__ == "0.7.0" and b"0.7.0" in _lib.lib().pcgrl_version()
