"""Microstructure levels on the device (control_pcgrl_amd.microstructure.MicrostructureEvaluator,
csrc/microstructure/pcgrl_microstructure.h): the kernel against the fixtures recorded from the reference
(tests/golden/microstructure) and against the plain-Python rules (tests/microstructure_rules.py) on generated maps
(tests/microstructure_levels.py); the measures and the diversity against tests/measures_numpy.py with T = 2.  Every output is
compared bit for bit, the doubles as their 64-bit patterns."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest
import torch

import measures_numpy as mn
from fixture_cases import fixture_cases
import microstructure_levels as ML
import microstructure_rules as R
from control_pcgrl_amd import _lib
from control_pcgrl_amd.microstructure import MicrostructureEvaluator, microstructure_config

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "microstructure")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))
CASES, CASE_IDS = fixture_cases(FILES)  # each file as ever, and split into several launches
DEV = "cuda:0"
T = 2
# maps per shape: fewer where the plain-Python rules are slow
GENERATED = [(8, 8, 400), (5, 9, 400), (33, 17, 120), (64, 64, 64)]


@functools.lru_cache(maxsize=None)
def maps_and_rules(h, w, n, seed=11):
    """n generated maps (random at 40-70 % empty, and the extremes in front) and what the rules say about each; computed once
    per shape and shared: the tests copy before they change a map."""
    rng = np.random.default_rng(seed + h * 100 + w)
    front = [ML.all_solid(h, w), ML.all_empty(h, w), ML.checkerboard(h, w), ML.checkerboard(h, w, False), ML.serpentine(h, w),
             ML.one_cell(h, w, h - 1, w - 1), ML.random_map(rng, h, w, 0.15), ML.random_map(rng, h, w, 0.9)]
    maps = np.stack(front + [ML.random_map(rng, h, w) for _ in range(n - len(front))])
    return maps, tuple(R.regions(m) for m in maps)


def expect(maps, regions, cap, weights=None):
    """The evaluator's outputs, as the rules give them from the regions of each map."""
    n = len(maps)
    out = {"stats": np.zeros((n, 2)), "loss": np.zeros(n), "regions": np.zeros(n, np.int32), "error": np.zeros(n, np.int32)}
    if cap:
        out["region_rec"] = np.full((n, cap, 5), -1, np.int16)
        out["region_tort"] = np.zeros((n, cap))
    for i, regs in enumerate(regions):
        if regs:
            out["stats"][i] = [max(r[4] for r in regs), R.numpy_mean([r[5] for r in regs])]
        out["loss"][i] = R.loss(out["stats"][i], weights)
        out["regions"][i] = len(regs)
        for j, r in enumerate(regs[:cap]):
            out["region_rec"][i, j] = r[:5]
            out["region_tort"][i, j] = r[5]
    out["path_length"], out["tortuosity"] = out["stats"][:, 0], out["stats"][:, 1]
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same(got, want, what=""):
    assert set(got) == set(want), (set(got), set(want))
    for k in want:
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape)
        bad = np.nonzero((bits(g) != bits(want[k])).reshape(len(g), -1).any(axis=1))[0]
        assert bad.size == 0, (what, k, "maps", bad[:8].tolist(), g[bad[0]].tolist(), want[k][bad[0]].tolist())


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("path,max_levels", CASES, ids=CASE_IDS)
def test_kernel_equals_fixtures(path, max_levels):
    z = np.load(path)
    grids = z["grids"]
    n, cap = len(grids), z["region_rec"].shape[1]
    stats = z["stats_bits"].view(np.float64)
    want = {"stats": stats, "loss": np.array([R.loss(s) for s in stats]), "regions": z["regions"],
            "error": np.zeros(n, np.int32), "region_rec": z["region_rec"], "region_tort": z["region_tort_bits"].view(np.float64),
            "path_length": stats[:, 0], "tortuosity": stats[:, 1]}
    with MicrostructureEvaluator(grids.shape[1:], DEV, **({"max_levels": max_levels} if max_levels else {})) as ev:
        assert_same(ev.evaluate(grids, region_cap=cap), want, os.path.basename(path))
        ev.check_errors()


@pytest.mark.parametrize("h,w,n", GENERATED, ids=[f"{h}x{w}" for h, w, _ in GENERATED])
def test_kernel_equals_rules_on_generated_maps(h, w, n):
    maps, regions = maps_and_rules(h, w, n)
    cap = max(len(r) for r in regions) + 1  # every region of every map, and one entry past the last
    with MicrostructureEvaluator((h, w), DEV) as ev:
        assert_same(ev.evaluate(maps, region_cap=cap), expect(maps, regions, cap), f"{h}x{w}")
        ev.check_errors()


def test_region_cap_zero_three_and_above_the_count():
    maps, regions = maps_and_rules(5, 9, 400)
    assert max(len(r) for r in regions) > 3 > min(len(r) for r in regions)
    with MicrostructureEvaluator((5, 9), DEV) as ev:
        full = ev.evaluate(maps, region_cap=40)
        assert_same(full, expect(maps, regions, 40))
        cut = ev.evaluate(maps, region_cap=3)
        assert_same(cut, expect(maps, regions, 3))
        assert torch.equal(cut["stats"], full["stats"]) and torch.equal(cut["regions"], full["regions"])  # the totals stay complete
        none = ev.evaluate(maps)
        assert "region_rec" not in none and "region_tort" not in none
        assert_same(none, expect(maps, regions, 0))


def test_skipped_buffers_stay_untouched():
    """through the C ABI: with region_cap = 0 the record buffers are not written even when given, and with every optional
    output null only the statistics are"""
    maps, regions = maps_and_rules(5, 9, 400)
    n = 70
    L = _lib.lib()
    g = torch.from_numpy(maps[:n].copy()).to(DEV)
    stats = torch.empty((n, 2), dtype=torch.float64, device=DEV)
    rec = torch.full((n, 4, 5), 77, dtype=torch.int16, device=DEV)
    tort = torch.full((n, 4), 7.5, dtype=torch.float64, device=DEV)
    cfg = microstructure_config((5, 9))
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.pcgrl_microstructure_evaluate(C.byref(cfg), n, g.data_ptr(), 0, stats.data_ptr(), None, None, rec.data_ptr(),
                                               tort.data_ptr(), None, stream))
    torch.cuda.synchronize()
    want = expect(maps[:n], regions[:n], 0)["stats"]
    assert_same({"stats": stats}, {"stats": want})
    assert (rec == 77).all() and (tort == 7.5).all()
    # the record without the values, and the values without the record
    stats.zero_()
    _lib.check(L.pcgrl_microstructure_evaluate(C.byref(cfg), n, g.data_ptr(), 4, stats.data_ptr(), None, None, rec.data_ptr(),
                                               None, None, stream))
    torch.cuda.synchronize()
    want4 = expect(maps[:n], regions[:n], 4)
    assert_same({"stats": stats, "region_rec": rec}, {"stats": want, "region_rec": want4["region_rec"]})
    assert (tort == 7.5).all()
    rec.fill_(77)
    _lib.check(L.pcgrl_microstructure_evaluate(C.byref(cfg), n, g.data_ptr(), 4, stats.data_ptr(), None, None, None,
                                               tort.data_ptr(), None, stream))
    torch.cuda.synchronize()
    assert_same({"region_tort": tort}, {"region_tort": want4["region_tort"]})
    assert (rec == 77).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(n):
    maps, regions = maps_and_rules(8, 8, 400)
    with MicrostructureEvaluator((8, 8), DEV) as ev:
        assert_same(ev.evaluate(maps[:n], region_cap=5), expect(maps[:n], regions[:n], 5), f"n={n}")


def test_batches_above_max_levels_run_as_successive_launches():
    maps, regions = maps_and_rules(8, 8, 400)
    with MicrostructureEvaluator((8, 8), DEV, max_levels=3) as ev:
        assert_same(ev.evaluate(maps[:8], region_cap=5), expect(maps[:8], regions[:8], 5))


@pytest.mark.parametrize("h,w,n", [(33, 17, 120), (64, 64, 64), (5, 9, 400)], ids=["33x17", "64x64", "5x9"])
def test_unaligned_grid_pointers(h, w, n):
    maps, regions = maps_and_rules(h, w, n)
    n = min(n, 40)
    want = expect(maps[:n], regions[:n], 6)
    with MicrostructureEvaluator((h, w), DEV) as ev:
        for off in (1, 3, 8, 15):
            buf = torch.zeros(n * h * w + 16, dtype=torch.uint8, device=DEV)
            g = buf[off:off + n * h * w].view(n, h, w)
            g.copy_(torch.from_numpy(maps[:n].copy()))
            assert g.data_ptr() % 16 == (buf.data_ptr() + off) % 16
            assert_same(ev.evaluate(g, region_cap=6), want, f"offset {off}")
            mm = ev.measures(g)
            assert np.array_equal(_np(mm.counts), mn.counts(maps[:n], T)), off


def test_tile_ids_above_1_read_as_solid_and_set_the_error_bit():
    maps, regions = maps_and_rules(8, 8, 400)
    dirty = maps[:16].copy()
    dirty[5, 3, 4] = 2
    dirty[9, 0, 0] = 255
    dirty[9, 7, 7] = 2
    clean = dirty.copy()
    clean[clean > 1] = 1  # read as solid
    want = expect(clean, tuple(R.regions(m) for m in clean), 8)
    want["error"][[5, 9]] = 1
    with MicrostructureEvaluator((8, 8), DEV) as ev:
        assert_same(ev.evaluate(dirty, region_cap=8), want)  # the rest of the batch is unaffected
        with pytest.raises(ValueError):
            ev.check_errors()
        ev.check_errors()  # cleared: raises once


def test_custom_weights():
    maps, regions = maps_and_rules(5, 9, 400)
    w = {"tortuosity": 0.3, "path-length": 5}
    with MicrostructureEvaluator((5, 9), DEV, weights=w) as ev:
        got = ev.evaluate(maps)
        want = expect(maps, regions, 0, w)
        assert_same(got, want)
    assert (want["loss"] != expect(maps, regions, 0)["loss"]).any()


@pytest.mark.parametrize("h,w,n", [(5, 9, 400), (64, 64, 64)], ids=["5x9", "64x64"])
def test_measures_and_diversity_against_the_numpy_rules(h, w, n):
    maps, _ = maps_and_rules(h, w, n)
    with MicrostructureEvaluator((h, w), DEV) as ev:
        m = ev.measures(maps)
        cnt, mat = mn.counts(maps, T), mn.matches(maps, T)
        assert m.counts.dtype == torch.int32 and tuple(m.counts.shape) == (n, T) and tuple(m.forms.shape) == (n, 5 + T)
        assert np.array_equal(_np(m.counts), cnt) and np.array_equal(_np(m.match), mat)
        bc = mn.bc_from_integers(cnt, mat, h, w, T)
        assert set(m.bc) == set(mn.BC_NAMES)
        for key in mn.BC_NAMES:
            assert np.array_equal(bits(_np(m.bc[key])), bits(np.asarray(bc[key], np.float64))), key
        assert np.array_equal(bits(_np(m.tile_fractions)), bits(mn.tile_fractions(cnt, h * w)))
        m0 = ev.measures(maps, entropy=False)
        assert m0.entropy is None and torch.equal(m0.forms, m.forms)
        for K in (n, 8):
            d = ev.diversity(maps, group=None if K == n else K, pairwise=True)
            S, near, idx, mats = mn.diversity(maps, T, K)
            assert np.array_equal(_np(d.hamming_sum), S) and np.array_equal(_np(d.nearest), near)
            assert np.array_equal(_np(d.nearest_idx), idx) and np.array_equal(_np(d.pairwise), mats)
            assert np.array_equal(bits(_np(d.div_score)), bits(mn.div_score(S, K, h * w)))
            assert np.array_equal(bits(_np(d.diversity_bonus)), bits(mn.diversity_bonus(S, K, h * w)))
        # ids are masked to one bit and set no error
        odd = maps[:8].copy()
        odd[0, 0, 0] = 2 + maps[0, 0, 0]
        assert torch.equal(ev.measures(odd).counts, ev.measures(maps[:8]).counts)
        ev.check_errors()


def test_behaviour_vectors():
    maps, regions = maps_and_rules(5, 9, 400)
    want = expect(maps, regions, 0)
    with MicrostructureEvaluator((5, 9), DEV) as ev:
        meas = ev.measures(maps)
        b = ev.behaviour(maps, ("emptiness", "tortuosity"))
        assert b.dtype == torch.float64 and tuple(b.shape) == (len(maps), 2)
        assert torch.equal(b[:, 0], meas.bc["emptiness"]) and np.array_equal(bits(_np(b[:, 1])), bits(want["tortuosity"]))
        b = ev.behaviour(maps, ("symmetry", "path-length"))
        assert torch.equal(b[:, 0], meas.bc["symmetry"]) and np.array_equal(bits(_np(b[:, 1])), bits(want["path_length"]))
        assert (_np(ev.behaviour(maps, "NONE")) == 0).all() and tuple(ev.behaviour(maps, "NONE").shape) == (len(maps), 1)
        # only what the names need is launched
        calls = []
        ev.evaluate = lambda *a, **k: calls.append("evaluate")
        assert torch.equal(ev.behaviour(maps, ("entropy", "NONE"))[:, 0], meas.bc["entropy"]) and not calls
        with pytest.raises(ValueError):
            ev.behaviour(maps, ("regions",))


def test_evaluate_under_graph_capture():
    maps, regions = maps_and_rules(8, 8, 400)
    static = torch.from_numpy(maps[:96].copy()).to(DEV)
    with MicrostructureEvaluator((8, 8), DEV, max_levels=64) as ev:
        eager = {k: v.clone() for k, v in ev.evaluate(static, region_cap=4).items()}
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            ev.evaluate(static, region_cap=4)
        torch.cuda.current_stream(DEV).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = ev.evaluate(static, region_cap=4)
        for k in ("stats", "loss", "regions", "region_rec", "region_tort", "error"):
            captured[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(captured[k], eager[k]), k
        assert_same(captured, expect(maps[:96], regions[:96], 4))
        # replayed on changed input
        static.copy_(torch.from_numpy(maps[96:192].copy()))
        graph.replay()
        torch.cuda.synchronize()
        assert_same(captured, expect(maps[96:192], regions[96:192], 4))
        ev.check_errors()
