"""The routes behind a Lode Runner level's path-length on the device (LodeRunnerEvaluator.routes,
csrc/loderunner/pcgrl_loderunner_routes.h): the kernel against the lists recorded from the reference
(tests/golden/loderunner_routes) and against the plain-Python rules' play(m, record=...) on generated levels.  Every output is
compared bit for bit; what routes() shares with evaluate() is compared with evaluate() as 64-bit patterns."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest
import torch

from fixture_cases import fixture_cases
import loderunner_levels as LL
import loderunner_routes_expect as X
import loderunner_rules as R
from control_pcgrl_amd import _lib
from control_pcgrl_amd.loderunner import LodeRunnerEvaluator, loderunner_config

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loderunner_routes")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))
CASES, CASE_IDS = fixture_cases(FILES)  # each file as ever, and split into several launches
DEV = "cuda:0"
ROUTE_KEYS = ("coords", "moves", "tour_len", "gold_off", "gold_back")
EVAL_KEYS = ("stats", "loss", "play", "gold_state", "gold_dist", "error")
# name: (H, W, maps): 300 of each kind at the stock size, 300 mixed ones at the small shapes, 6 at the largest
GENERATED = {"gold": (8, 12, 300), "structured": (8, 12, 300), "random": (8, 12, 300), "4x4": (4, 4, 300), "1x5": (1, 5, 300),
             "5x7": (5, 7, 300), "16x32": (16, 32, 6)}


@functools.lru_cache(maxsize=None)
def levels_and_pairs(name):
    """generated maps and the rules' counted pairs of each; computed once and shared: a test copies before it changes a map"""
    h, w, n = GENERATED[name]
    maps = LL.batch(name, X.GOLD_KIND_SEED, n, h, w) if name in LL.KINDS else LL.mixed(1, n, h, w)
    return maps, tuple(X.pairs_of_rules(m) for m in maps)


def cap_for(pairs):
    return max(1, max((j + 1 for p in pairs for j, _, _ in p), default=1))


def assert_routes(got, pairs, gold_cap, route_cap, what="", moves=True):
    want = X.expect(pairs, gold_cap, route_cap, moves)
    for k in ROUTE_KEYS:
        if k not in want:
            assert k not in got, k
            continue
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape)
        bad = np.nonzero((g != want[k]).reshape(len(g), -1).any(axis=1))[0]
        assert bad.size == 0, (what, k, "levels", bad[:8].tolist(), g[bad[0]].tolist(), want[k][bad[0]].tolist())


def assert_same_as_evaluate(got, ev_out):
    for k in EVAL_KEYS:
        if k not in ev_out:
            assert k not in got, k
            continue
        a, b = got[k], ev_out[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype == torch.float64:
            a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
        assert torch.equal(a, b), k


@pytest.mark.parametrize("path,max_levels", CASES, ids=CASE_IDS)
def test_kernel_equals_the_recorded_lists(path, max_levels):
    z = np.load(path)
    grids = z["grids"]
    pairs = [X.pairs_of_fixture(z, i) for i in range(len(grids))]
    cap = max(cap_for(pairs), int((grids == R.GOLD).reshape(len(grids), -1).sum(1).max()), 1)
    with LodeRunnerEvaluator(grids.shape[1:], DEV, **({"max_levels": max_levels} if max_levels else {})) as ev:
        got = ev.routes(grids, gold_cap=cap, moves=True)
        assert_routes(got, pairs, cap, 8 * grids.shape[1] * grids.shape[2], os.path.basename(path))
        assert_same_as_evaluate(got, ev.evaluate(grids, gold_cap=cap))
        for i in range(len(grids)):
            assert LodeRunnerEvaluator.split_routes(got, i) == X.split(pairs[i])
        ev.check_errors()


@pytest.mark.parametrize("name", list(GENERATED))
def test_kernel_equals_rules_on_generated_levels(name):
    maps, pairs = levels_and_pairs(name)
    h, w, _ = GENERATED[name]
    if name == "gold":  # the comparison is not empty: seed 1 gives 152 levels with a route, 6 with a counted gold at index >= 32
        with_route = sum(1 for p in pairs if p)
        over_32 = sum(1 for p in pairs if any(j >= 32 for j, _, _ in p))
        print(f"gold-kind 8 x 12: {with_route} levels with a route, {over_32} with a counted gold at index >= 32")
        assert with_route >= 100 and over_32 >= 3
    cap = cap_for(pairs)
    with LodeRunnerEvaluator((h, w), DEV) as ev:
        got = ev.routes(maps, gold_cap=cap, moves=True)
        assert_routes(got, pairs, cap, 8 * h * w, name)
        assert_same_as_evaluate(got, ev.evaluate(maps, gold_cap=cap))
        ev.check_errors()


def test_route_cap_cuts_the_cells_and_keeps_the_totals():
    maps, pairs = levels_and_pairs("gold")
    maps, pairs = maps[:64], pairs[:64]
    tour = max(sum(len(a[0]) + len(b[0]) for _, a, b in p) for p in pairs)
    assert tour > 8 and sum(1 for p in pairs if p) > 8
    cap = cap_for(pairs)
    with LodeRunnerEvaluator((8, 12), DEV) as ev:
        full = ev.routes(maps, gold_cap=cap, moves=True)
        for route_cap in (0, 1, tour - 1, tour, tour + 1):
            got = ev.routes(maps, gold_cap=cap, route_cap=route_cap, moves=True)
            assert got["coords"].shape == (64, route_cap, 2) and got["moves"].shape == (64, route_cap)
            assert_routes(got, pairs, cap, route_cap, f"route_cap={route_cap}")  # the prefix, and -1 behind a shorter tour
            for k in ("tour_len", "gold_off", "gold_back") + EVAL_KEYS:
                assert torch.equal(got[k], full[k]), (route_cap, k)
        lengths = ev.routes(maps, gold_cap=0, route_cap=0)  # sizes a second call
        assert set(lengths) == {"stats", "loss", "play", "tour_len", "coords", "error", "win", "path_length"}
        assert int(lengths["tour_len"].max()) == tour


def test_gold_cap_below_the_gold_count_leaves_the_cells():
    maps, pairs = levels_and_pairs("gold")
    maps, pairs = maps[:64], pairs[:64]
    assert min(int((m == R.GOLD).sum()) for m in maps) > 3 and any(j >= 3 for p in pairs for j, _, _ in p)
    with LodeRunnerEvaluator((8, 12), DEV) as ev:
        full = ev.routes(maps, gold_cap=cap_for(pairs), moves=True)
        cut = ev.routes(maps, gold_cap=3, moves=True)
        assert_routes(cut, pairs, 3, 8 * 96, "gold_cap=3")
        for k in ("coords", "moves", "tour_len", "stats", "play"):
            assert torch.equal(cut[k], full[k]), k
        assert_same_as_evaluate(cut, ev.evaluate(maps, gold_cap=3))


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(n):
    maps, pairs = levels_and_pairs("gold")
    with LodeRunnerEvaluator((8, 12), DEV) as ev:
        assert_routes(ev.routes(maps[:n], gold_cap=48, moves=True), pairs[:n], 48, 8 * 96, f"n={n}")


def test_more_levels_than_blocks():
    """above 4096 levels a block strides over several levels on one workspace slot: a lane's chain of one level must be read
    before its search of the next overwrites it.  The 300 maps, repeated"""
    maps, pairs = levels_and_pairs("4x4")
    maps, pairs = np.concatenate([maps] * 15), pairs * 15
    assert len(maps) == 4500
    with LodeRunnerEvaluator((4, 4), DEV, max_levels=4500) as ev:
        assert_routes(ev.routes(maps, gold_cap=8, route_cap=64, moves=True), pairs, 8, 64)


def test_batches_above_max_levels_run_as_successive_launches():
    maps, pairs = levels_and_pairs("gold")
    with LodeRunnerEvaluator((8, 12), DEV, max_levels=3) as ev:
        got = ev.routes(maps[:8], gold_cap=48, moves=True)
        assert_routes(got, pairs[:8], 48, 8 * 96)
        assert_same_as_evaluate(got, ev.evaluate(maps[:8], gold_cap=48))


def test_levels_without_a_tour():
    maps, _ = levels_and_pairs("gold")
    maps = maps[:3].copy()
    maps[0][maps[0] == R.PLAYER] = R.EMPTY  # no player
    free = np.argwhere(maps[1] == R.EMPTY)
    maps[1][tuple(free[0])] = R.PLAYER  # two players
    maps[2][maps[2] == R.GOLD] = R.EMPTY  # no gold
    pairs = [X.pairs_of_rules(m) for m in maps]
    assert pairs == [[], [], []]
    with LodeRunnerEvaluator((8, 12), DEV) as ev:
        got = ev.routes(maps, gold_cap=8, route_cap=5, moves=True)
        assert_routes(got, pairs, 8, 5)
        assert got["tour_len"].tolist() == [0, 0, 0] and bool((got["coords"] == -1).all()) and bool((got["gold_off"] == -1).all())
        assert got["stats"][:, 3].tolist() == [0.0, 0.0, -1.0]
        assert LodeRunnerEvaluator.split_routes(got, 2) == []


def test_tile_id_above_7_reads_as_empty_and_sets_the_error_bit():
    maps, _ = levels_and_pairs("gold")
    dirty = maps[:16].copy()
    dirty[5, 3, 4] = 9
    clean = dirty.copy()
    clean[5, 3, 4] = 0
    pairs = [X.pairs_of_rules(m) for m in clean]
    with LodeRunnerEvaluator((8, 12), DEV) as ev:
        got = ev.routes(dirty, gold_cap=48, moves=True)
        assert_routes(got, pairs, 48, 8 * 96)
        assert got["error"].tolist() == [0] * 5 + [1] + [0] * 10
        with pytest.raises(ValueError):
            ev.check_errors()
        ev.check_errors()  # cleared


def test_dirty_workspace():
    maps, pairs = levels_and_pairs("gold")
    with LodeRunnerEvaluator((8, 12), DEV) as ev:
        first = {k: v.clone() for k, v in ev.routes(maps[:256], gold_cap=48, moves=True).items()}
        for ones in (-1, 0x01010101):  # every bit set; every byte 1
            ev._workspace.fill_(ones)
            second = ev.routes(maps[:256], gold_cap=48, moves=True)
            for k in first:
                assert torch.equal(first[k], second[k]), (ones, k)
        assert_routes(second, pairs[:256], 48, 8 * 96)


def test_every_optional_output_null_in_turn():
    maps, pairs = levels_and_pairs("gold")
    n, gold_cap, route_cap = 70, 48, 200
    L = _lib.lib()
    g = torch.from_numpy(maps[:n].copy()).to(DEV)
    nbytes = L.pcgrl_loderunner_workspace_bytes(n, 8, 12)
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=DEV)
    cfg = loderunner_config((8, 12))
    shapes = {"stats": ((n, 5), torch.float64), "loss": ((n,), torch.float64), "play": ((n, 4), torch.int32),
              "gold_state": ((n, gold_cap), torch.int8), "gold_dist": ((n, gold_cap), torch.int16),
              "gold_off": ((n, gold_cap), torch.int32), "gold_back": ((n, gold_cap), torch.int16),
              "coords": ((n, route_cap, 2), torch.int16), "moves": ((n, route_cap), torch.int8), "tour_len": ((n,), torch.int32),
              "error": ((n,), torch.int32)}

    def run(without, rcap=route_cap):
        out = {k: torch.full(s, 77, dtype=t, device=DEV) for k, (s, t) in shapes.items()}
        p = {k: (None if k == without else v.data_ptr()) for k, v in out.items()}
        _lib.check(L.pcgrl_loderunner_routes(C.byref(cfg), n, g.data_ptr(), ws.data_ptr(), nbytes, gold_cap, rcap, p["stats"],
                                             p["loss"], p["play"], p["gold_state"], p["gold_dist"], p["gold_off"], p["gold_back"],
                                             p["coords"], p["moves"], p["tour_len"], p["error"],
                                             torch.cuda.current_stream().cuda_stream), "pcgrl_loderunner_routes")
        torch.cuda.synchronize()
        return out

    full = run(None)
    assert_routes(full, pairs[:n], gold_cap, route_cap)
    with LodeRunnerEvaluator((8, 12), DEV) as ev:
        assert_same_as_evaluate(full, ev.evaluate(g, gold_cap=gold_cap))
    for without in shapes:
        if without in ("stats", "coords"):  # (stats is required; coords may be null only with route_cap == 0, below)
            continue
        got = run(without)
        for k in shapes:
            if k == without:
                assert bool((got[k] == 77).all()), k  # untouched
            else:
                assert torch.equal(got[k], full[k]), (without, k)
    got = run("coords", rcap=0)
    for k in ("stats", "tour_len", "gold_off", "gold_back", "gold_state"):
        assert torch.equal(got[k], full[k]), k
    assert bool((got["coords"] == 77).all()) and bool((got["moves"] == 77).all())


def test_routes_captured_and_replayed_on_a_side_stream():
    maps, pairs = levels_and_pairs("gold")
    static = torch.from_numpy(maps[:96].copy()).to(DEV)
    with LodeRunnerEvaluator((8, 12), DEV, max_levels=64) as ev:
        eager = {k: v.clone() for k, v in ev.routes(static, gold_cap=48, moves=True).items()}
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            ev.routes(static, gold_cap=48, moves=True)
        torch.cuda.current_stream(DEV).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = ev.routes(static, gold_cap=48, moves=True)
        for k in ROUTE_KEYS + EVAL_KEYS:
            captured[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(captured[k], eager[k]), k
        assert_routes(captured, pairs[:96], 48, 8 * 96)
        ev.check_errors()
