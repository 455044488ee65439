"""The 3-D holey dungeon and maze levels on the device (control_pcgrl_amd.mc3d_holey.Mc3dHoleyEvaluator,
csrc/mc3d_holey/pcgrl_mc3d_holey.h): the kernel against the fixtures recorded from the reference (tests/golden/mc3d_holey) and
against the plain-Python rules (tests/mc3d_holey_rules.py) on generated levels (tests/mc3d_holey_levels.py).  Everything is
compared exactly; the loss as its 64-bit pattern."""
import functools
import os

import numpy as np
import pytest
import torch

import mc3d_holey_levels as Lv
import mc3d_holey_rules as R
from control_pcgrl_amd import Mc3dHoleyEvaluator, archive_for
from control_pcgrl_amd.archive import placed_cells

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mc3d_holey")
DEV = "cuda:0"
PROBLEMS = ("dungeon", "maze")
# (interior shape, terrain levels, random levels): the stock sizes, the smallest, a non-cubic one, the largest; 7^3 keeps the
# per-cell search state in LDS and 15^3 / 16^3 keep it in the workspace
GENERATED = [((3, 3, 3), 48, 16), ((3, 4, 5), 48, 16), ((7, 7, 7), 64, 16), ((15, 15, 15), 8, 2), ((16, 16, 16), 8, 2)]
FIELDS = ("stats", "loss", "error", "play", "route_len", "leg_len", "route2_len")


def expect(problem, grids, holes, cap=None):
    """what the rules say about each level, as the arrays evaluate() returns (cap None: ample, the longest route's length)"""
    res = [R.evaluate(problem, grids[i], holes[i]) for i in range(len(grids))]
    n, (Z, Y, X) = len(grids), grids.shape[1:]
    longest = max([1] + [max(len(r["route"]), len(r["route2"])) for r in res])
    cap = longest if cap is None else cap
    out = {"stats": np.array([r["stats"] for r in res], np.int32), "loss": np.array([r["loss"] for r in res], np.float64),
           "error": np.array([r["error"] for r in res], np.int32), "play": np.array([r["play"] for r in res], np.int32),
           "route_len": np.array([len(r["route"]) for r in res], np.int32),
           "leg_len": np.array([r["leg_len"] for r in res], np.int32),
           "route2_len": np.array([len(r["route2"]) for r in res], np.int32)}
    for key, src in (("coords", "route"), ("coords2", "route2")):
        a = np.full((n, max(cap, 1), 3), -1, np.int16)
        for i, r in enumerate(res):
            t = np.array(r[src][:cap], np.int16).reshape(-1, 3)
            a[i, :len(t)] = t
        out[key] = a[:, :cap]
    for key, src in (("overlay", "overlay"), ("overlay2", "overlay2")):
        a = np.zeros((n, Z + 2, Y + 2, X + 2), bool)
        for i, r in enumerate(res):
            for x, y, z in r[src]:
                a[i, z, y, x] = True
        out[key] = a
    out["cap"], out["res"] = cap, res
    return out


@functools.lru_cache(maxsize=None)
def generated(problem, shape, n_terrain, n_random):
    """a set of terrain levels, then random ones, and what the rules say; computed once per case and shared (read only)"""
    seed = 41 + 7 * shape[0] + shape[2] + (1000 if problem == "maze" else 0)
    tg, th = Lv.structured_set(problem, shape, n_terrain, seed)
    rg, rh = Lv.random_set(problem, shape, n_random, seed + 1)
    grids, holes = np.concatenate([tg, rg]), np.concatenate([th, rh])
    return grids, holes, expect(problem, grids, holes)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same(got, want, lo=0, hi=None, fields=FIELDS, tag=""):
    for k in fields:
        g, w = got[k].cpu().numpy(), want[k][lo:hi]
        where = np.argwhere(bits(g) != bits(w))
        assert where.size == 0, f"{tag}{k}: first difference at {where[0]}: got {g[tuple(where[0])]}, want {w[tuple(where[0])]}"


def run(ev, grids, holes, **kw):
    out = ev.evaluate(torch.from_numpy(np.ascontiguousarray(grids)).to(DEV), torch.from_numpy(np.ascontiguousarray(holes)).to(DEV),
                      **kw)
    torch.cuda.synchronize()
    return out


def load_fixture(problem):
    z = np.load(os.path.join(GOLDEN, problem + ".npz"))
    levels, at = [], 0
    for i, shape in enumerate(z["shapes"]):
        size = int(np.prod(shape))
        rec = {"name": str(z["names"][i]), "grid": z["grids"][at:at + size].reshape(shape), "holes": z["holes"][i],
               "stats": z["stats"][i], "leg_len": z["leg_len"][i]}
        for k in ("route", "route2", "overlay", "overlay2"):
            rec[k] = z[k][z[k + "_off"][i]:z[k + "_off"][i + 1]]
        levels.append(rec)
        at += size
    return levels


@pytest.mark.parametrize("problem", PROBLEMS)
def test_fixtures_every_field(problem):
    levels = load_fixture(problem)
    for shape in sorted({tuple(int(s) for s in lv["grid"].shape) for lv in levels}):
        group = [lv for lv in levels if lv["grid"].shape == shape]
        cap = max([1] + [max(len(lv["route"]), len(lv["route2"])) for lv in group])
        with Mc3dHoleyEvaluator(problem, shape, DEV) as ev:
            out = run(ev, np.stack([lv["grid"] for lv in group]), np.stack([lv["holes"] for lv in group]), route_cap=cap,
                      overlay=True)
            ev.check_errors()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        for i, lv in enumerate(group):
            tag = f"{problem} {lv['name']}"
            assert got["stats"][i].tolist() == lv["stats"].tolist(), tag
            assert got["error"][i] == 0, tag
            assert got["leg_len"][i].tolist() == lv["leg_len"].tolist(), tag
            for key, ln, src in (("coords", "route_len", "route"), ("coords2", "route2_len", "route2")):
                assert got[ln][i] == len(lv[src]), tag
                assert np.array_equal(got[key][i, :len(lv[src])], lv[src]), (tag, key)
                assert (got[key][i, len(lv[src]):] == -1).all(), (tag, key)
            for key in ("overlay", "overlay2"):
                cells = sorted((int(x), int(y), int(z)) for z, y, x in np.argwhere(got[key][i]))
                assert cells == [tuple(int(v) for v in t) for t in lv[key]], (tag, key)
            assert bits(got["loss"][i:i + 1])[0] == bits(np.array([R.loss_of(problem, lv["stats"].tolist())]))[0], tag


@pytest.mark.parametrize("shape,n_terrain,n_random", GENERATED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
@pytest.mark.parametrize("problem", PROBLEMS)
def test_generated_levels_against_the_rules(problem, shape, n_terrain, n_random):
    grids, holes, want = generated(problem, shape, n_terrain, n_random)
    # the sets are worth their time: from the rules alone, at least half of the terrain levels connect
    reached = sum(Lv.connected(problem, r) for r in want["res"][:n_terrain])
    assert 2 * reached >= n_terrain, (reached, n_terrain)
    with Mc3dHoleyEvaluator(problem, shape, DEV) as ev:
        out = run(ev, grids, holes, route_cap=want["cap"], overlay=True)
        assert_same(out, want, fields=FIELDS + ("coords", "coords2", "overlay", "overlay2"))
        ev.check_errors()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_batch_sizes(problem, n):
    grids, holes, want = generated(problem, (3, 4, 5), 257, 0)
    with Mc3dHoleyEvaluator(problem, (3, 4, 5), DEV, max_blocks=64) as ev:  # 257 levels: the blocks stride over them
        out = run(ev, grids[:n], holes[:n], route_cap=want["cap"], overlay=True)
        assert_same(out, want, 0, n, fields=FIELDS + ("coords", "coords2", "overlay", "overlay2"))


@pytest.mark.parametrize("problem", PROBLEMS)
def test_grids_one_byte_into_an_allocation(problem):
    grids, holes, want = generated(problem, (7, 7, 7), 64, 16)
    n, size = len(grids), grids[0].size
    raw = torch.zeros(n * size + 1, dtype=torch.uint8, device=DEV)
    raw[1:] = torch.from_numpy(grids.reshape(-1)).to(DEV)
    view = raw[1:].view(n, 7, 7, 7)
    assert view.data_ptr() % 2 == 1
    with Mc3dHoleyEvaluator(problem, (7, 7, 7), DEV) as ev:
        out = ev.evaluate(view, torch.from_numpy(holes).to(DEV))
        torch.cuda.synchronize()
        assert_same(out, want)


@pytest.mark.parametrize("problem", PROBLEMS)
def test_refused_holes_and_unknown_tiles_in_a_batch(problem):
    grids, holes, want = generated(problem, (3, 4, 5), 48, 16)
    grids, holes = grids.copy(), holes.copy()
    Z, Y, X = 3, 4, 5
    bad = {3: [[1, 0, 0], [1, 3, X + 1]],      # on an edge
           10: [[0, 2, 0], [1, 3, X + 1]],     # z = 0
           11: [[1, 2, 0], [Z, 3, X + 1]],     # z = Z: the head would leave through the top border
           20: [[1, 2, 2], [1, 3, X + 1]],     # inside
           21: [[1, 2, 0], [1, 3, X + 5]],     # outside the map
           47: [[1, 2, 0], [-1, 3, X + 1]]}
    for i, h in bad.items():
        holes[i] = np.array(h, np.int32)
    grids[5, 1, 2, 3] = 7  # an id neither problem knows: read as DIRT
    mixed = expect(problem, grids, holes)
    for i in bad:
        assert mixed["error"][i] & R.ERR_HOLE and (mixed["stats"][i] == -1).all() and mixed["loss"][i] == -np.inf
    assert mixed["error"][5] & R.ERR_TILE
    with Mc3dHoleyEvaluator(problem, (3, 4, 5), DEV) as ev:
        out = run(ev, grids, holes, route_cap=mixed["cap"], overlay=True)
        assert_same(out, mixed, fields=FIELDS + ("coords", "coords2", "overlay", "overlay2"))
        keep = [i for i in range(len(grids)) if i not in bad and i != 5]  # the neighbours answer as they did alone
        for k in FIELDS:
            assert np.array_equal(bits(out[k].cpu().numpy()[keep]), bits(want[k][keep])), k
        with pytest.raises(ValueError, match="tile id"):
            ev.check_errors()


@pytest.mark.parametrize("problem", PROBLEMS)
def test_route_caps(problem):
    grids, holes, want = generated(problem, (7, 7, 7), 64, 16)
    assert want["cap"] > 6
    with Mc3dHoleyEvaluator(problem, (7, 7, 7), DEV) as ev:
        out = run(ev, grids, holes)
        assert "coords" not in out and "overlay" not in out
        assert_same(out, want)
        for cap in (5, want["cap"] + 9):
            out = run(ev, grids, holes, route_cap=cap)
            assert_same(out, want)  # the lengths are complete whatever the cap cuts
            for key in ("coords", "coords2"):
                full = np.concatenate([want[key], np.full((len(grids), 9, 3), -1, np.int16)], 1)[:, :cap]
                assert np.array_equal(out[key].cpu().numpy(), full), (key, cap)


@pytest.mark.parametrize("problem", PROBLEMS)
def test_two_runs_and_a_side_stream(problem):
    grids, holes, want = generated(problem, (7, 7, 7), 64, 16)
    g, h = torch.from_numpy(grids).to(DEV), torch.from_numpy(holes).to(DEV)
    with Mc3dHoleyEvaluator(problem, (7, 7, 7), DEV) as ev:
        a = ev.evaluate(g, h, route_cap=want["cap"], overlay=True)
        b = ev.evaluate(g, h, route_cap=want["cap"], overlay=True)
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            c = ev.evaluate(g, h, route_cap=want["cap"], overlay=True)
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
            assert torch.equal(a[k].view(torch.uint8), c[k].view(torch.uint8)), k
        assert_same(c, want, fields=FIELDS + ("coords", "coords2", "overlay", "overlay2"))


@pytest.mark.parametrize("problem", PROBLEMS)
def test_evaluate_under_graph_capture(problem):
    grids, holes, want = generated(problem, (7, 7, 7), 64, 16)
    n, cap = 20, want["cap"]
    sg, sh = torch.from_numpy(grids[:n].copy()).to(DEV), torch.from_numpy(holes[:n].copy()).to(DEV)
    fields = FIELDS + ("coords", "coords2", "overlay", "overlay2")
    with Mc3dHoleyEvaluator(problem, (7, 7, 7), DEV) as ev:
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            ev.evaluate(sg, sh, route_cap=cap, overlay=True)
        torch.cuda.current_stream(DEV).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = ev.evaluate(sg, sh, route_cap=cap, overlay=True)
        for lo in (0, 20, 40, 60):  # the capture's own inputs, then three replays on changed ones
            sg.copy_(torch.from_numpy(grids[lo:lo + n].copy()))
            sh.copy_(torch.from_numpy(holes[lo:lo + n].copy()))
            for k in fields:
                captured[k].zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert_same(captured, want, lo, lo + n, fields=fields, tag=f"replay at {lo}: ")
        ev.check_errors()


@pytest.mark.parametrize("problem", PROBLEMS)
def test_one_generation_through_the_archive(problem):
    grids, holes, want = generated(problem, (7, 7, 7), 64, 16)
    names = ["path-length", "n_jump"]
    with Mc3dHoleyEvaluator(problem, (7, 7, 7), DEV) as ev:
        with pytest.raises(NotImplementedError, match="2-D"):
            ev.behaviour(grids, holes, ["emptiness"])
        with pytest.raises(ValueError):
            ev.behaviour(grids, holes, ["brightness"])
        bc = ev.behaviour(grids, holes, names + ["NONE"])
        cols = [ev.stat_keys.index(k) for k in names]
        assert np.array_equal(bc.cpu().numpy(), np.concatenate([want["stats"][:, cols], np.zeros((len(grids), 1))], 1))
        arc = archive_for(ev, names, bins=8)
        assert arc.map_shape == (7, 7, 7) and arc.map_bytes == 343 and arc.n_tiles == ev.spec.n_tiles
        loss = ev.evaluate(grids, holes)["loss"]
        g = torch.from_numpy(grids).to(DEV)
        arc.add(g, loss, bc[:, :2])
        cells = placed_cells(want["stats"][:, cols].astype(np.float64), arc.dims, arc.bounds)
        assert arc.stats().count == len(set(cells.tolist()))
        children, parents = arc.ask(32, seed=5)
        assert tuple(children.shape) == (32, 7, 7, 7) and int(children.max()) < ev.spec.n_tiles
        assert set(parents.cpu().tolist()) <= set(cells.tolist())
        again = ev.evaluate(children, holes[:32])  # the next generation evaluates without leaving the device
        torch.cuda.synchronize()
        assert (again["error"].cpu().numpy() == 0).all()
