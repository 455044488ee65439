"""The quality-diversity grid archive on the device (include/pcgrl_amd_archive.h) against the sequential
restatement (tests/archive_rules.py) and the numpy twins of control_pcgrl_amd/archive.py.  Every comparison is exact but
stats().sum, which is held to math.fsum within cells * 2^-53 * sum |x|."""
import math
import os

import numpy as np
import pytest
import torch

import archive_rules as R
import loderunner_rules as LR
import measures_numpy as mn
from conftest import GOLDEN
from control_pcgrl_amd import DeviceGridArchive, LodeRunnerEvaluator, archive, archive_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUNDS, DIMS, placement_values = R.BOUNDS, R.DIMS, R.placement_values
SIZES = [1, 63, 64, 65, 257, 4096]


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _fsum(values):
    try:
        return math.fsum(values)
    except (ValueError, OverflowError):
        return math.nan


def same(arc, ref, what=""):
    """the whole device archive against the restatement: objectives, behaviours, flags, maps, stats() and elites()"""
    d = arc.dense()
    assert np.array_equal(_np(d.occupied), ref.flag), what
    assert np.array_equal(_bits(_np(d.objectives)), _bits(ref.obj)), what
    assert np.array_equal(_bits(_np(d.behaviours)), _bits(ref.beh)), what
    assert np.array_equal(_np(d.grids), ref.maps), what
    occ = ref.occupied()
    st = arc.stats()
    o = ref.obj[occ]
    assert st.count == len(occ), what
    if len(occ):
        assert st.max == o.max() and st.min == o.min(), what
        want = _fsum(o.tolist())
        if math.isfinite(want):
            assert abs(st.sum - want) <= ref.cells * 2.0 ** -53 * _fsum(np.abs(o).tolist()), (what, st.sum, want)
        else:
            assert st.sum == want or (math.isnan(st.sum) and math.isnan(want)), (what, st.sum, want)
    else:
        assert (st.max, st.min, st.sum) == (-math.inf, math.inf, 0.0), what
    el = arc.elites()
    assert np.array_equal(_np(el.cells), occ) and np.array_equal(_bits(_np(el.objectives)), _bits(o)), what
    assert np.array_equal(_bits(_np(el.behaviours)), _bits(ref.beh[occ])) and np.array_equal(_np(el.grids), ref.maps[occ]), what


def add_both(arc, ref, grids, obj, beh=None, cells=None, what="", refused=False):
    """one batch into the device archive and into the restatement; every output compared"""
    out = arc.add(torch.as_tensor(grids).to(DEV), torch.as_tensor(np.asarray(obj, np.float64)).to(DEV),
                  None if beh is None else torch.as_tensor(np.asarray(beh, np.float64)).to(DEV),
                  None if cells is None else torch.as_tensor(np.asarray(cells, np.int32)).to(DEV))
    status, cell, counts = ref.add(grids, np.asarray(obj, np.float64), beh, cells)
    assert np.array_equal(_np(out.status), status), (what, _np(out.status), status)
    assert np.array_equal(_np(out.cell), cell), what
    assert np.array_equal(_np(out.counts), counts), (what, _np(out.counts), counts)
    if refused:
        assert (status == 3).any()
        with pytest.raises(ValueError, match="refused"):
            arc.check_errors()
    arc.check_errors()
    same(arc, ref, what)
    return status


def pair(dims, bounds, map_shape=(2, 3), T=8):
    return DeviceGridArchive(dims, bounds, map_shape, T, device=DEV), R.SeqArchive(dims, bounds, map_shape)


def _maps(rng, n, shape=(2, 3), T=8):
    return rng.integers(0, T, (n,) + tuple(shape), dtype=np.uint8)


# ---- placement --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(1,), (100, 100), (7, 3, 5), (2, 2, 2, 2)])
def test_placement(dims):
    rng = np.random.default_rng(len(dims))
    bounds = [BOUNDS[j % 3] for j in range(len(dims))]
    cols = []
    for j, d in enumerate(dims):
        lo, hi = bounds[j]
        v = np.concatenate([placement_values(lo, hi, d), *[placement_values(lo, hi, k) for k in DIMS]])
        if (lo, hi) == (0.0, 95.0):
            v = np.concatenate([v, np.arange(96.0)])
        if (lo, hi) == (0.0, 1.0):
            v = np.concatenate([v, np.arange(97) / 96.0])
        cols.append(v)
    n = 4 * max(len(c) for c in cols)
    beh = np.stack([np.resize(c, n) if j == 0 else rng.permutation(np.resize(c, n)) for j, c in enumerate(cols)], 1)
    beh[5, len(dims) - 1] = math.nan
    beh[6], beh[7] = [b[1] for b in bounds], [b[0] for b in bounds]
    arc, ref = pair(dims, bounds)
    want = np.array([-1 if (c := R.place(b, dims, bounds)) is None else c for b in beh], np.int32)
    assert want[5] == -1 and want[6] == ref.cells - 1 and want[7] == 0
    assert np.array_equal(_np(arc.cell_of(torch.as_tensor(beh).to(DEV))), want)
    assert np.array_equal(archive.placed_cells(beh, dims, bounds), want)
    arc.check_errors()  # cell_of sets no error bit
    add_both(arc, ref, _maps(rng, n), rng.integers(0, 3, n).astype(np.float64), beh, what=dims, refused=True)
    arc.close()


def test_cells_passed_directly():
    rng = np.random.default_rng(1)
    arc, ref = pair((7, 3, 5), [BOUNDS[0]] * 3)
    n = 300
    cells = rng.integers(0, 105, n)
    add_both(arc, ref, _maps(rng, n), rng.integers(0, 3, n).astype(np.float64), cells=cells, what="cells")
    assert (ref.beh == 0).all()  # no behaviours were given: zeros are stored
    # cells with behaviours: the behaviours are stored, not placed
    beh = rng.random((n, 3)) * 5 - 2
    add_both(arc, ref, _maps(rng, n), rng.integers(2, 5, n).astype(np.float64), beh, cells=cells[::-1].copy(), what="cells + beh")
    cells[[0, 7, 299]] = [-1, 105, 1 << 30]
    status = add_both(arc, ref, _maps(rng, n), np.full(n, 9.0), cells=cells, what="cells out of range", refused=True)
    assert status[[0, 7, 299]].tolist() == [3, 3, 3] and (status != 3).sum() == n - 3
    arc.close()


# ---- insertion --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_insertion_one_cell(n):
    rng = np.random.default_rng(n)
    mid = np.full((n, 1), 0.5)
    for what, obj in (("equal", np.full(n, 1.25)), ("increasing", np.arange(n) * 0.5 - 3), ("decreasing", -np.arange(n) * 0.25)):
        arc, ref = pair((1,), [(0, 1)])
        status = add_both(arc, ref, _maps(rng, n), obj, mid, what=(what, n))
        assert status[0 if what != "increasing" else n - 1] == 2 and (status != 0).sum() == 1, what
        arc.close()
    # -inf takes an empty cell and then replaces nothing; +inf replaces, and then stays
    arc, ref = pair((1,), [(0, 1)])
    assert add_both(arc, ref, _maps(rng, n), np.full(n, -math.inf), mid, what="-inf")[0] == 2
    assert not add_both(arc, ref, _maps(rng, n), np.full(n, -math.inf), mid, what="-inf again").any()
    obj = np.full(n, -1.0)
    obj[n // 2] = math.inf
    assert add_both(arc, ref, _maps(rng, n), obj, mid, what="+inf")[n // 2] == 1
    assert not add_both(arc, ref, _maps(rng, n), np.full(n, math.inf), mid, what="+inf again").any()
    arc.close()
    # -0.0 against an occupant 0.0, and the reverse
    for first, second in ((0.0, -0.0), (-0.0, 0.0)):
        arc, ref = pair((1,), [(0, 1)])
        add_both(arc, ref, _maps(rng, n), np.full(n, first), mid, what="zero")
        assert not add_both(arc, ref, _maps(rng, n), np.full(n, second), mid, what="other zero").any()
        assert math.copysign(1, ref.obj[0]) == math.copysign(1, first)
        arc.close()


@pytest.mark.parametrize("n", SIZES)
def test_insertion_random_and_refilled(n):
    rng = np.random.default_rng(100 + n)
    arc, ref = pair((4, 4), [(0, 1), (0, 95)])
    values = np.array([-2.0, 0.5, 3.0])
    beh = np.stack([rng.random(n), rng.integers(0, 96, n).astype(np.float64)], 1)
    add_both(arc, ref, _maps(rng, n), values[rng.integers(0, 3, n)], beh, what=("random", n))
    add_both(arc, ref, _maps(rng, n), values[rng.integers(0, 3, n)], beh[::-1].copy(), what=("random again", n))
    # candidates that equal the occupants replace none; nextafter above replaces all
    occ = ref.occupied()
    m = len(occ)
    status = add_both(arc, ref, _maps(rng, m), ref.obj[occ].copy(), ref.beh[occ].copy(), what=("equal to the occupants", n))
    assert not status.any()
    status = add_both(arc, ref, _maps(rng, m), np.nextafter(ref.obj[occ], np.inf), ref.beh[occ].copy(), what=("nextafter", n))
    assert (status == 1).all()
    # refused candidates: the others are handled as if the refused ones were absent
    obj = values[rng.integers(0, 3, n)] + 10
    beh2 = beh.copy()
    bad_o, bad_b = rng.integers(0, n), rng.integers(0, n)
    obj[bad_o] = math.nan
    beh2[bad_b, 1] = math.nan
    keep = np.ones(n, bool)
    keep[[bad_o, bad_b]] = False
    twin = ref.copy()
    grids = _maps(rng, n)
    status = add_both(arc, ref, grids, obj, beh2, what=("refused", n), refused=True)
    assert (status[~keep] == 3).all()
    if keep.any():
        s2, _, _ = twin.add(grids[keep], obj[keep], beh2[keep])
        assert np.array_equal(s2, status[keep])
    assert np.array_equal(twin.flag, ref.flag) and np.array_equal(_bits(twin.obj), _bits(ref.obj))
    assert np.array_equal(twin.maps, ref.maps)
    arc.close()


@pytest.mark.parametrize("L", [1, 77, 96, 1856, 4096])
def test_map_bytes(L):
    rng = np.random.default_rng(L)
    arc, ref = pair((4, 4), [(0, 1), (0, 1)], (L,), 256)
    n = 65
    grids = rng.integers(0, 256, (n, L), dtype=np.uint8)
    beh, obj = rng.random((n, 2)), rng.integers(0, 3, n).astype(np.float64)
    # the caller's maps start one byte into an allocation
    buf = torch.zeros(n * L + 17, dtype=torch.uint8, device=DEV)
    view = buf[1:1 + n * L].view(n, L)
    view.copy_(torch.as_tensor(grids))
    assert view.data_ptr() % 16 == 1
    out = arc.add(view, torch.as_tensor(obj).to(DEV), torch.as_tensor(beh).to(DEV))
    status, cell, counts = ref.add(grids, obj, beh)
    assert np.array_equal(_np(out.status), status) and np.array_equal(_np(out.counts), counts)
    same(arc, ref, L)
    assert not buf[0].item() and not buf[1 + n * L:].any().item()
    # an aligned batch takes the 16-byte loads when L is a multiple of 16
    add_both(arc, ref, rng.integers(0, 256, (n, L), dtype=np.uint8), obj + 1, beh[::-1].copy(), what=("aligned", L))
    kids, parent = arc.ask(33, seed=L, rate=0.5)
    occ = ref.occupied()
    p = occ[archive.sampled_parents(L, 0, 33, len(occ))]
    assert np.array_equal(_np(parent), p) and np.array_equal(_np(kids), archive.mutated(ref.maps[p], L, 0, 0.5, 256))
    arc.close()


def test_reproducible_images():
    rng = np.random.default_rng(9)
    n = 4096
    grids, obj = _maps(rng, n, (8, 12)), rng.integers(0, 4, n).astype(np.float64)
    beh = np.stack([rng.random(n), rng.integers(0, 96, n).astype(np.float64)], 1)
    images = []
    for _ in range(2):
        arc = DeviceGridArchive((10, 10), [(0, 1), (0, 95)], (8, 12), 8, device=DEV)
        arc.add(torch.as_tensor(grids).to(DEV), torch.as_tensor(obj).to(DEV), torch.as_tensor(beh).to(DEV))
        images.append(_np(arc.state_dict()["image"]))
        assert len(images[-1]) == arc.state_bytes
        arc.close()
    assert images[0].tobytes() == images[1].tobytes()


# ---- selection and mutation -------------------------------------------------------------------------------------------------

def _filled(rng, k, T, map_shape=(8, 12)):
    """an archive of 4 x 4 with its first k cells occupied"""
    arc, ref = pair((4, 4), [(0, 1), (0, 1)], map_shape, T)
    cells = rng.permutation(16)[:k]
    add_both(arc, ref, _maps(rng, k, map_shape, T), rng.random(k), cells=cells, what="fill")
    return arc, ref


@pytest.mark.parametrize("k,T,rate", [(1, 8, 0.01), (7, 8, 0.01), (16, 8, 0.01), (7, 1, 1.0), (7, 2, 1.0), (16, 2, 0.01),
                                      (7, 8, 0.0), (16, 8, 1.0)])
def test_ask_equals_the_twins(k, T, rate):
    rng = np.random.default_rng(k * 100 + T)
    arc, ref = _filled(rng, k, T)
    occ = ref.occupied()
    for draw, n in enumerate((257, 64, 4096)):  # three consecutive calls: the counter advances
        kids, parent = arc.ask(n, seed=77, rate=rate)
        p = occ[archive.sampled_parents(77, draw, n, k)]
        assert np.array_equal(_np(parent), p), (draw, n)
        want = archive.mutated(ref.maps[p], 77, draw, rate, T)
        assert np.array_equal(_np(kids), want), (draw, n)
        if rate == 1.0 and T > 1:
            assert (want != ref.maps[p]).all()
        if rate == 0.0 or T == 1:
            assert (want == ref.maps[p]).all()
    arc.check_errors()
    same(arc, ref, "ask leaves the archive alone")
    arc.close()


def test_ask_on_an_empty_archive():
    arc, ref = pair((4, 4), [(0, 1), (0, 1)], (8, 12), 8)
    grids = torch.full((5, 8, 12), 201, dtype=torch.uint8, device=DEV)
    parent = torch.full((5,), -7, dtype=torch.int32, device=DEV)
    arc.ask(5, out=(grids, parent))
    with pytest.raises(RuntimeError, match="empty archive"):
        arc.check_errors()
    assert (grids == 201).all().item() and (parent == -7).all().item()
    arc.check_errors()
    # nothing was drawn: the first ask of the filled archive is draw 0
    rng = np.random.default_rng(0)
    add_both(arc, ref, _maps(rng, 3, (8, 12)), [1.0, 2.0, 3.0], cells=[3, 9, 4])
    kids, parent = arc.ask(5, seed=1, out=(grids, parent))
    assert kids is grids and np.array_equal(_np(parent), ref.occupied()[archive.sampled_parents(1, 0, 5, 3)])
    arc.close()


def test_add_and_ask_in_one_graph():
    rng = np.random.default_rng(4)
    arc, ref = pair((4, 4), [(0, 1), (0, 95)], (8, 12), 8)
    n = 257
    grids = torch.as_tensor(_maps(rng, n, (8, 12))).to(DEV)
    obj = torch.as_tensor(rng.integers(0, 3, n).astype(np.float64)).to(DEV)
    beh = torch.as_tensor(np.stack([rng.random(n), rng.integers(0, 96, n).astype(np.float64)], 1)).to(DEV)
    kids = torch.zeros((n, 8, 12), dtype=torch.uint8, device=DEV)
    parent = torch.zeros(n, dtype=torch.int32, device=DEV)
    arc.add(grids, obj, beh)  # eager once: nothing is allocated during the capture but torch's own outputs
    arc.ask(n, seed=3, out=(kids, parent))
    ref.add(_np(grids), _np(obj), _np(beh))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = arc.add(grids, obj, beh)
        arc.ask(n, seed=3, out=(kids, parent))
    for replay in range(3):
        # a new batch through the same tensors: the graph adds it, then draws from the archive that holds it
        g2, o2 = _maps(rng, n, (8, 12)), rng.integers(0, 3, n).astype(np.float64) + replay + 1
        b2 = np.stack([rng.random(n), rng.integers(0, 96, n).astype(np.float64)], 1)
        grids.copy_(torch.as_tensor(g2)), obj.copy_(torch.as_tensor(o2)), beh.copy_(torch.as_tensor(b2))
        graph.replay()
        torch.cuda.synchronize()
        status, cell, counts = ref.add(g2, o2, b2)
        assert np.array_equal(_np(out.status), status) and np.array_equal(_np(out.cell), cell)
        assert np.array_equal(_np(out.counts), counts)
        occ = ref.occupied()
        p = occ[archive.sampled_parents(3, 1 + replay, n, len(occ))]  # (the eager ask was draw 0)
        assert np.array_equal(_np(parent), p), replay
        assert np.array_equal(_np(kids), archive.mutated(ref.maps[p], 3, 1 + replay, 0.01, 8)), replay
    arc.check_errors()
    same(arc, ref, "after the replays")
    arc.close()


def test_side_stream():
    rng = np.random.default_rng(6)
    arc, ref = pair((4, 4), [(0, 1), (0, 95)], (8, 12), 8)
    n = 4096
    g, o = _maps(rng, n, (8, 12)), rng.integers(0, 3, n).astype(np.float64)
    b = np.stack([rng.random(n), rng.integers(0, 96, n).astype(np.float64)], 1)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out = arc.add(torch.as_tensor(g).to(DEV), torch.as_tensor(o).to(DEV), torch.as_tensor(b).to(DEV))
        kids, parent = arc.ask(n, seed=8)
        st = arc.stats(sync=False)
    side.synchronize()
    status, cell, counts = ref.add(g, o, b)
    assert np.array_equal(_np(out.status), status) and np.array_equal(_np(out.cell), cell) and np.array_equal(_np(out.counts), counts)
    occ = ref.occupied()
    p = occ[archive.sampled_parents(8, 0, n, len(occ))]
    assert np.array_equal(_np(parent), p) and np.array_equal(_np(kids), archive.mutated(ref.maps[p], 8, 0, 0.01, 8))
    assert _np(st)[0] == len(occ) and _np(st)[1] == ref.obj[occ].max()
    with torch.cuda.stream(side):
        arc.check_errors()
    same(arc, ref, "side stream")
    arc.close()


# ---- the image --------------------------------------------------------------------------------------------------------------

def test_image_round_trip_and_refusals():
    rng = np.random.default_rng(12)
    arc, ref = _filled(rng, 7, 8)
    arc.ask(10, seed=5)
    arc.ask(10, seed=5)  # the counter is 2
    state = arc.state_dict()
    assert state["image"].numel() == arc.state_bytes and state["dims"] == (4, 4)
    fresh = DeviceGridArchive((4, 4), [(0, 1), (0, 1)], (8, 12), 8, device=DEV)
    fresh.load_state_dict(state)
    same(fresh, ref, "restored")
    assert _np(fresh.state_dict()["image"]).tobytes() == _np(state["image"]).tobytes()
    # on through one more add and ask: both archives go the same way, at draw 2
    g, o, b = _maps(rng, 65, (8, 12)), rng.random(65) + 0.5, rng.random((65, 2))
    ref2 = ref.copy()
    add_both(arc, ref, g, o, b, what="original")
    add_both(fresh, ref2, g, o, b, what="restored copy")
    k1, p1 = arc.ask(65, seed=5)
    k2, p2 = fresh.ask(65, seed=5)
    occ = ref.occupied()
    p = occ[archive.sampled_parents(5, 2, 65, len(occ))]
    assert np.array_equal(_np(p1), p) and np.array_equal(_np(p2), p)
    assert np.array_equal(_np(k1), _np(k2)) and np.array_equal(_np(k1), archive.mutated(ref.maps[p], 5, 2, 0.01, 8))
    # an image of other dims, another map length, other bounds or another tile count: refused, the target unchanged
    for kw in (dict(dims=(4, 5)), dict(map_shape=(8, 11)), dict(bounds=[(0, 1), (0, 2)]), dict(n_tiles=7), dict(dims=(16,), bounds=[(0, 1)])):
        args = dict(dims=(4, 4), bounds=[(0, 1), (0, 1)], map_shape=(8, 12), n_tiles=8)
        args.update(kw)
        other = DeviceGridArchive(device=DEV, **args)
        oref = R.SeqArchive(args["dims"], args["bounds"], args["map_shape"])
        add_both(other, oref, _maps(rng, 9, args["map_shape"], 7), rng.random(9), cells=np.arange(9))
        before = _np(other.state_dict()["image"]).tobytes()
        with pytest.raises(ValueError, match="pcgrl_archive_import"):
            other.load_state_dict(state)
        assert _np(other.state_dict()["image"]).tobytes() == before
        same(other, oref, kw)
        other.close()
    with pytest.raises(ValueError):
        fresh.load_state_dict({"image": state["image"][:-16]})
    same(fresh, ref2, "after a short image")
    arc.close(), fresh.close()


# ---- with an evaluator ------------------------------------------------------------------------------------------------------

def test_archive_for_every_evaluator():
    from control_pcgrl_amd import DDaveEvaluator, MDungeonEvaluator, MicrostructureEvaluator, SmbEvaluator, VecPcgrlEnv
    cases = [(LodeRunnerEvaluator(device=DEV), ["emptiness", "path-length"], [(0.0, 1.0), (0.0, 103.0)], (8, 12), 8),
             (SmbEvaluator(device=DEV), ["sol-length", "symmetry"], [(0.0, 348.0), (0.0, 1.0)], (16, 116), 7),
             (MicrostructureEvaluator((16, 16), device=DEV), ["tortuosity"], None, (16, 16), 2),
             (DDaveEvaluator(device=DEV), ["entropy", "co-occurance"], [(0.0, 1.0)] * 2, (7, 11), 7),
             (MDungeonEvaluator(device=DEV), ["symmetry-vertical"], [(0.0, 1.0)], (11, 7), 8),
             (VecPcgrlEnv("binary", "narrow", (16, 16), 4, device=DEV), ["regions", "path-length"], [(0.0, 128.0), (0.0, 136.0)],
              (16, 16), 2)]
    for e, names, bounds, shape, T in cases:
        arc = archive_for(e, names, bins=5)
        assert arc.dims == (5,) * len(names) and arc.map_shape == shape and arc.n_tiles == T and arc.stats().count == 0
        if bounds is not None:
            assert list(arc.bounds) == bounds
        else:
            assert list(arc.bounds) == [tuple(float(v) for v in e.spec.cond_bounds[k]) for k in names]
        with pytest.raises(Exception, match="not found in self.bc_bounds"):
            archive_for(e, names + ["brightness"])
        arc.close()
        e.close()
    env3 = VecPcgrlEnv("minecraft_3D_maze", "narrow", (7, 7, 7), 2, device=DEV)
    with pytest.raises(NotImplementedError, match="2-D maps only"):
        archive_for(env3, ["path-length"])
    env3.close()


def test_a_lode_runner_generation_stays_on_the_device():
    z = np.load(os.path.join(GOLDEN, "loderunner", "stock_random.npz"))
    grids, stats = z["grids"], z["stats"]
    n = len(grids)
    assert n == 64
    names = ["emptiness", "path-length"]
    ev = LodeRunnerEvaluator((8, 12), device=DEV)
    arc = archive_for(ev, names)
    assert arc.dims == (100, 100) and arc.bounds == ((0.0, 1.0), (0.0, 103.0))
    ref = R.SeqArchive(arc.dims, arc.bounds, (8, 12))
    g = torch.as_tensor(grids).to(DEV)
    out = arc.add(g, -ev.evaluate(g, gold_cap=0)["loss"], ev.behaviour(g, names))
    # the restatement is fed the recorded statistics
    cnt, mat = mn.counts(grids, 8), mn.matches(grids, 8)
    beh = np.stack([dict(mn.bc_from_integers(cnt, mat, 8, 12, 8))["emptiness"], stats[:, 4]], 1)
    obj = np.array([-LR.loss(s) for s in stats])
    status, cell, counts = ref.add(grids, obj, beh)
    assert np.array_equal(_np(out.status), status) and np.array_equal(_np(out.cell), cell) and np.array_equal(_np(out.counts), counts)
    assert counts[0] > 8 and counts[2] == 0
    same(arc, ref, "recorded levels")
    # one generation, nothing copied to the host until it is over
    kids, parent = arc.ask(n, seed=21, rate=0.05)
    res = ev.evaluate(kids, gold_cap=0)
    kb = ev.behaviour(kids, names)
    out = arc.add(kids, -res["loss"], kb)
    occ = ref.occupied()
    p = occ[archive.sampled_parents(21, 0, n, len(occ))]
    want_kids = archive.mutated(ref.maps[p], 21, 0, 0.05, 8)
    assert np.array_equal(_np(parent), p) and np.array_equal(_np(kids), want_kids) and (want_kids != ref.maps[p]).any()
    kstats = _np(res["stats"])
    assert np.array_equal(_bits(_np(res["loss"])), _bits([LR.loss(s) for s in kstats]))
    kcnt, kmat = mn.counts(want_kids, 8), mn.matches(want_kids, 8)
    want_beh = np.stack([dict(mn.bc_from_integers(kcnt, kmat, 8, 12, 8))["emptiness"], kstats[:, 4]], 1)
    assert np.array_equal(_bits(_np(kb)), _bits(want_beh))
    status, cell, counts = ref.add(want_kids, -_np(res["loss"]), want_beh)
    assert np.array_equal(_np(out.status), status) and np.array_equal(_np(out.cell), cell) and np.array_equal(_np(out.counts), counts)
    same(arc, ref, "after one generation")
    arc.check_errors(), ev.check_errors()
    arc.close(), ev.close()
