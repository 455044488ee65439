"""The 3-D NCA level generator on the device (include/pcgrl_amd_nca3d.h) against its numpy twins
(control_pcgrl_amd/nca3d.py): levels, n_step, frames and the error bits are equal bit for bit.  What runs: 3 x 3 x 3 (every
cell on the ring), 3 x 4 x 5 and 5 x 4 x 3 (strides, axis order), 7 x 7 x 7 (two passes of 192 lanes, the second ragged),
16 x 16 x 16 (the largest image), T in {2, 3, 5, 8}, both modes, shared and per-genome init, shared and per-seed holes; the
recorded reference roll-outs; the genome that tells tap order from tile order; the refusals; graphs and streams; and the chains
with Mc3dHoleyEvaluator and the genome archive."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import evo_rules as E
import nca3d_reference as r3
from conftest import GOLDEN
from nca3d_reference import genomes, seeds
from control_pcgrl_amd import (Mc3dHoleyEvaluator, Nca3dGenerator, NcaEvolution, all_holes, archive, evo, fixed_holes,
                               generator3d_for, genome_archive_for, mc3d_holey_score, nca3d)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (map shape, T, holey, n_steps, G, S, per-genome init, per-seed holes)
CASES = [((3, 3, 3), 2, False, 10, 3, 4, False, False), ((3, 3, 3), 5, True, 10, 3, 4, True, True),
         ((3, 4, 5), 3, False, 10, 3, 4, True, False), ((3, 4, 5), 8, True, 4, 2, 3, False, False),
         ((5, 4, 3), 5, True, 10, 3, 4, False, True), ((5, 4, 3), 2, False, 2, 3, 4, True, False),
         ((7, 7, 7), 5, True, 10, 6, 4, True, True), ((7, 7, 7), 8, False, 4, 2, 2, False, False),
         ((7, 7, 7), 3, True, 1, 2, 3, False, False),
         ((16, 16, 16), 2, True, 3, 1, 1, False, False), ((16, 16, 16), 8, False, 2, 1, 1, False, False)]


def _np(t):
    return t.cpu().numpy()


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def device_run(gen, weights, init, holes=None, n_steps=None, frames=True, out=None):
    return gen.generate(_t(weights), _t(init), holes=None if holes is None else _t(np.asarray(holes, np.int32)), n_steps=n_steps,
                        frames=frames, out=out)


def same(out, want, what=""):
    assert np.array_equal(_np(out.n_step), want.n_step), (what, _np(out.n_step), want.n_step)
    assert np.array_equal(_np(out.levels), want.levels), what
    if out.frames is not None:
        assert np.array_equal(_np(out.frames), want.frames), what


def some_holes(rng, shape, S):
    """S pairs of all_holes(shape), the first and the last among them"""
    pairs = all_holes(shape)
    pick = np.concatenate([[0, len(pairs) - 1], rng.integers(0, len(pairs), max(S - 2, 0))])[:S]
    return pairs[pick]


@functools.lru_cache(maxsize=None)
def case(i):
    shape, T, holey, n_steps, G, S, per, per_seed = CASES[i]
    rng = np.random.default_rng(4400 + i)
    w = genomes(rng, G, T)
    init = seeds(rng, (G, S) if per else (S,), shape, T)
    holes = None if not holey else (some_holes(rng, shape, S) if per_seed else fixed_holes(shape))
    return w, init, holes, nca3d.generated(w, init, holes, n_steps, n_tiles=T)


def _id(c):
    return f"{c[0][0]}x{c[0][1]}x{c[0][2]}-T{c[1]}-{'holey' if c[2] else 'plain'}-n{c[3]}"


@pytest.mark.parametrize("i", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_device_equals_twin(i):
    shape, T, holey, n_steps, G, S, per, per_seed = CASES[i]
    w, init, holes, want = case(i)
    with Nca3dGenerator(T, shape, n_steps=n_steps, holey=holey, device=DEV) as gen:
        assert gen.n_params == w.shape[1] == nca3d.n_params(T)
        same(device_run(gen, w, init, holes), want, CASES[i])
        bare = device_run(gen, w, init, holes, frames=False)
        assert bare.frames is None
        same(bare, want, CASES[i])
        assert gen.poll_errors() == want.error_bits == 0
    assert (want.n_step >= 0).all()


def test_holes_change_the_levels():
    """the same genomes and seeds under two hole pairs and in plain mode: the ring is read"""
    shape, T = (5, 4, 3), 5
    w, init, _, _ = case(4)
    pairs = all_holes(shape)
    a = nca3d.generated(w, init, pairs[0], 10, n_tiles=T)
    b = nca3d.generated(w, init, pairs[-1], 10, n_tiles=T)
    c = nca3d.generated(w, init, None, 10, n_tiles=T)
    assert not np.array_equal(a.levels, c.levels) and not np.array_equal(a.frames, b.frames)
    with Nca3dGenerator(T, shape, holey=True, device=DEV) as gen:
        same(device_run(gen, w, init, pairs[0]), a)
        same(device_run(gen, w, init, pairs[-1]), b)
    with Nca3dGenerator(T, shape, device=DEV) as gen:
        same(device_run(gen, w, init), c)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "nca3d", "*.npz"))), ids=os.path.basename)
def test_reference_fixtures_on_the_device(path):
    """every recorded step at every non-exempt cell (one step from the reference's own map: n_steps = 1), and the clean
    trajectories end to end"""
    z = np.load(path)
    T, n_steps, holey = int(z["n_tiles"]), int(z["n_steps"]), bool(z["holey"])
    shape = z["init"].shape[1:]
    with Nca3dGenerator(T, shape, n_steps=n_steps, holey=holey, device=DEV) as gen:
        for hi in range(len(z["hole_pairs"]) if holey else 1):
            of_pair = (z["hole"] == hi) if holey else np.ones(len(z["init"]), bool)
            holes = z["hole_pairs"][hi] if holey else None
            rows = np.flatnonzero(z["clean"] & of_pair)
            if len(rows):
                out = device_run(gen, z["weights"][z["genome"][rows]], z["init"][rows][:, None], holes)
                assert np.array_equal(_np(out.n_step)[:, 0], z["n_step"][rows])
                assert np.array_equal(_np(out.frames)[:, 0], z["frames"][rows])
                assert np.array_equal(_np(out.levels)[:, 0], z["frames"][rows, -1])
            # single steps from the recorded maps
            prev = np.concatenate([z["init"][:, None], z["frames"][:, :-1]], axis=1)  # the map before step k
            live = (np.arange(n_steps)[None, :] <= z["n_step"][:, None]) & of_pair[:, None]
            idx = np.argwhere(live)
            one = device_run(gen, z["weights"][z["genome"][idx[:, 0]]], prev[idx[:, 0], idx[:, 1]][:, None], holes, n_steps=1,
                             frames=False)
            got = _np(one.levels)[:, 0]
            keep = ~z["exempt"][idx[:, 0], idx[:, 1]]
            assert keep.sum() > 0 and not (got != z["frames"][idx[:, 0], idx[:, 1]])[keep].any()
        gen.check_errors()


def test_the_order_is_by_tap():
    g, m = r3.order_genome(), r3.order_map()
    want = nca3d.generated(g[None], m[None], None, 1)
    assert want.levels[0, 0, 1, 1, 1] == 1  # (tile order would leave tile 0: tests/test_nca3d_cpu.py)
    with Nca3dGenerator(2, (3, 3, 3), n_steps=1, device=DEV) as gen:
        out = device_run(gen, g[None], m[None])
        same(out, want)
        assert _np(out.levels)[0, 0, 1, 1, 1] == 1


def test_pairs_stop_at_different_steps():
    """genomes of three sizes on shared seeds: some pairs stand still early, others run all steps, in one batch"""
    rng = np.random.default_rng(4420)
    T, shape = 2, (5, 4, 3)
    w = np.concatenate([genomes(rng, 6, T, scale=s) for s in (0.3, 1.0, 3.0)])
    init = seeds(rng, (4,), shape, T)
    want = nca3d.generated(w, init, fixed_holes(shape), 10, n_tiles=T)
    assert len(np.unique(want.n_step)) >= 3 and (want.n_step == 9).any() and (want.n_step < 9).any(), np.unique(want.n_step)
    with Nca3dGenerator(T, shape, holey=True, device=DEV) as gen:
        same(device_run(gen, w, init, fixed_holes(shape)), want)
        gen.check_errors()


def test_zero_weights():
    for holey in (False, True):
        with Nca3dGenerator(2, (7, 7, 7), holey=holey, device=DEV) as gen:
            holes = fixed_holes((7, 7, 7)) if holey else None
            zero = np.zeros((1, gen.n_params), np.float32)
            out = device_run(gen, zero, np.zeros((3, 7, 7, 7), np.uint8), holes)
            assert (_np(out.n_step) == 0).all() and (_np(out.levels) == 0).all() and (_np(out.frames) == 0).all()
            ones = np.ones((1, 7, 7, 7), np.uint8)  # every sigmoid 0.5: the first index wins once, then the map stands
            out = device_run(gen, zero, ones, holes)
            same(out, nca3d.generated(zero, ones, holes, 10))
            assert _np(out.n_step).tolist() == [[1]]
            gen.check_errors()


def overflow_genome(T=4):
    """tests/test_gpu_nca.py's, in 3-D: reads centre taps only.  A cell of tile 1 becomes 2, a cell of tile 2 becomes 3, a cell
    of tile 0 stays; at a cell of tile 3 units 0 and 1 are 3e38 each, layer 2 adds them to inf and layer 3 makes a NaN."""
    g = np.zeros(nca3d.n_params(T), np.float32)
    w = nca3d.unpack_weights(g, T)
    w.w1[3, 1, 1, 1, 1] = w.w2[3, 3] = w.w1[4, 2, 1, 1, 1] = w.w2[4, 4] = 1.0
    w.w3[2, 3] = w.w3[3, 4] = 2.0
    w.w1[0, 3, 1, 1, 1] = w.w1[1, 3, 1, 1, 1] = 3e38
    w.w2[0, 0] = w.w2[0, 1] = 1.0
    return g


def test_nonfinite_after_the_first_step():
    """the refusal overwrites the frame rows that valid steps wrote; the cell that overflows is in the second pass (7 x 7 x 7:
    cell 342 of 192 + 151), in the first, or is cell 0"""
    T, n_steps, shape, rng = 4, 6, (7, 7, 7), np.random.default_rng(4430)
    w = genomes(rng, 3, T)
    w[1] = overflow_genome(T)
    init = seeds(rng, (3, 4), shape, T)
    init[1] = 0
    init[1, 0, 6, 6, 6] = 1   # 1 -> 2 -> 3 -> overflow at step 2, in the last cell
    init[1, 1, 3, 3, 3] = 2   # 2 -> 3 -> overflow at step 1
    init[1, 2, 0, 0, 0] = 2   # the same in cell 0, with a tile 1 that is still on its way
    init[1, 2, 6, 0, 0] = 1
    want = nca3d.generated(w, init, None, n_steps, n_tiles=T)
    assert want.error_bits == nca3d.ERR_NONFINITE and want.n_step[1].tolist() == [-1, -1, -1, 0]
    assert (want.n_step[[0, 2]] >= 0).all() and (want.frames[1, :3] == init[1, :3, None]).all()
    with Nca3dGenerator(T, shape, n_steps=n_steps, device=DEV) as gen:
        out = device_run(gen, w, init)
        same(out, want)
        assert np.array_equal(_np(out.levels)[1], init[1]) and (_np(out.frames)[1] == init[1][:, None]).all()
        assert gen.poll_errors() == nca3d.ERR_NONFINITE and gen.poll_errors() == 0
        same(device_run(gen, w, init, frames=False), want)
        with pytest.raises(ValueError, match="non-finite"):
            gen.check_errors()
        gen.check_errors()  # cleared


def test_errors_leave_neighbours_alone():
    """a bad hole, a bad tile and a non-finite genome inside one batch: those pairs alone are refused"""
    rng = np.random.default_rng(4440)
    T, shape = 3, (5, 4, 3)
    w = genomes(rng, 3, T)
    w[1, nca3d.n_params(T) - 2 * 32 - T + 5] = np.inf  # l3.weight[1, 5] of genome 1
    init = seeds(rng, (3, 4), shape, T)
    init[2, 1, 4, 3, 2] = T  # a bad tile in the last cell of (genome 2, seed 1)
    holes = some_holes(rng, shape, 4).copy()
    holes[2, 1] = (5, 0, 1)  # seed 2: the exit's head would be in the top ring (z = Z)
    ok = some_holes(rng, shape, 4)
    assert not nca3d.hole_ok(holes[2, 1], shape)
    want = nca3d.generated(w, init, holes, 10, n_tiles=T)
    assert want.error_bits == (nca3d.ERR_TILE | nca3d.ERR_NONFINITE | nca3d.ERR_HOLE)
    assert want.n_step[1].tolist() == [-1] * 4 and want.n_step[2, 1] == -1 and (want.n_step[:, 2] == -1).all()
    assert (want.n_step >= 0).sum() == 5
    with Nca3dGenerator(T, shape, holey=True, device=DEV) as gen:
        out = device_run(gen, w, init, holes)
        same(out, want)
        assert np.array_equal(_np(out.levels)[:, 2], init[:, 2]) and (_np(out.frames)[:, 2] == init[:, 2, None]).all()
        with pytest.raises(ValueError, match="side face"):
            gen.check_errors()
        gen.check_errors()  # cleared
        # the other pairs are what they are without the bad one
        alone = device_run(gen, w[:1], init[:1], holes[[0, 1, 3]][[0, 1, 0, 2]])
        assert np.array_equal(_np(alone.levels)[0, [0, 1, 3]], _np(out.levels)[0, [0, 1, 3]])
        gen.poll_errors()
        # each bit on its own
        fine = genomes(rng, 1, T)
        device_run(gen, fine, init[2], ok)
        assert gen.poll_errors() == nca3d.ERR_TILE
        device_run(gen, w[1:2], init[1], ok)
        assert gen.poll_errors() == nca3d.ERR_NONFINITE
        for bad in ((0, 0, 1), (1, 0, 0), (1, 5, 4), (1, 2, 2), (-1, 0, 1), (2, 0, 4), (1, 1, 5)):  # (Z, Y, X) = (5, 4, 3)
            h = fixed_holes(shape).copy()
            h[0] = bad
            assert not nca3d.hole_ok(bad, shape)
            out = device_run(gen, fine, init[0], h)
            assert gen.poll_errors() == nca3d.ERR_HOLE, bad
            assert (_np(out.n_step) == -1).all() and np.array_equal(_np(out.levels)[0], init[0])


def test_out_reuse_and_argument_checks():
    rng = np.random.default_rng(4450)
    T, shape = 2, (3, 4, 5)
    P = nca3d.n_params(T)
    with Nca3dGenerator(T, shape, n_steps=4, device=DEV) as gen:
        w, init = genomes(rng, 2, T), seeds(rng, (3,), shape, T)
        out = device_run(gen, w, init)
        ptrs = (out.levels.data_ptr(), out.n_step.data_ptr(), out.frames.data_ptr())
        w2, init2 = genomes(rng, 2, T), seeds(rng, (2, 3), shape, T)
        again = device_run(gen, w2, init2, out=out)
        assert again is out and ptrs == (out.levels.data_ptr(), out.n_step.data_ptr(), out.frames.data_ptr())
        same(out, nca3d.generated(w2, init2, None, 4, n_tiles=T))
        with pytest.raises(ValueError, match="out.levels"):
            device_run(gen, genomes(rng, 3, T), init, out=out)
        with pytest.raises(ValueError, match=str(P)):
            device_run(gen, np.zeros((2, P - 1), np.float32), init)
        with pytest.raises(ValueError, match="float32"):
            device_run(gen, np.zeros((2, P), np.float64), init)
        with pytest.raises(ValueError, match="init_states"):
            device_run(gen, w, seeds(rng, (3,), (3, 5, 4), T))
        with pytest.raises(ValueError, match="n_steps"):
            device_run(gen, w, init, n_steps=1025)
        with pytest.raises(ValueError, match="takes no holes"):
            device_run(gen, w, init, fixed_holes(shape))
        gen.check_errors()
    with Nca3dGenerator(T, shape, holey=True, device=DEV) as holey:
        with pytest.raises(ValueError, match="needs holes"):
            device_run(holey, w, init)
        with pytest.raises(ValueError, match=r"holes must be"):
            device_run(holey, w, init, np.zeros((2, 2, 3), np.int32))
    with pytest.raises(ValueError, match=r"\[2, 8\]"):
        Nca3dGenerator(9, (7, 7, 7), device=DEV)
    with pytest.raises(ValueError, match=r"\[3, 16\]"):
        Nca3dGenerator(2, (7, 17, 7), device=DEV)
    with pytest.raises(ValueError, match=r"\[3, 16\]"):
        Nca3dGenerator(2, (2, 7, 7), device=DEV)
    with pytest.raises(RuntimeError, match="closed"):
        gen.generate(torch.zeros((1, P), device=DEV), torch.zeros((1,) + shape, dtype=torch.uint8, device=DEV))


def test_captured_graph_replays_on_new_inputs():
    rng = np.random.default_rng(4460)
    T, shape, G, S = 5, (5, 4, 3), 4, 3
    with Nca3dGenerator(T, shape, holey=True, device=DEV) as gen:
        w, init = _t(genomes(rng, G, T)), _t(seeds(rng, (S,), shape, T))
        holes = _t(some_holes(rng, shape, S))
        out = gen.generate(w, init, holes=holes, frames=True)  # eager once
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            gen.generate(w, init, holes=holes, frames=True, out=out)
        for replay in range(2):
            w2, i2, h2 = genomes(rng, G, T), seeds(rng, (S,), shape, T), some_holes(rng, shape, S)
            w.copy_(torch.as_tensor(w2)), init.copy_(torch.as_tensor(i2)), holes.copy_(torch.as_tensor(h2))
            graph.replay()
            torch.cuda.synchronize()
            same(out, nca3d.generated(w2, i2, h2, 10, n_tiles=T), replay)
        gen.check_errors()


def test_side_stream_and_second_run_are_byte_identical():
    rng = np.random.default_rng(4470)
    T, shape, G, S = 3, (7, 7, 7), 4, 3
    with Nca3dGenerator(T, shape, n_steps=8, holey=True, device=DEV) as gen:
        w, init, holes = _t(genomes(rng, G, T)), _t(seeds(rng, (G, S), shape, T)), _t(fixed_holes(shape))
        first = gen.generate(w, init, holes=holes, frames=True)
        second = gen.generate(w, init, holes=holes, frames=True)
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            third = gen.generate(w, init, holes=holes, frames=True)
            assert gen.poll_errors() == 0  # (synchronises the side stream)
        torch.cuda.current_stream(DEV).wait_stream(side)
        for other in (second, third):
            for name in ("levels", "n_step", "frames"):
                assert getattr(other, name).data_ptr() != getattr(first, name).data_ptr()
                assert torch.equal(getattr(other, name), getattr(first, name)), name
        same(first, nca3d.generated(_np(w), _np(init), _np(holes), 8, n_tiles=T))
        assert gen.poll_errors() == 0


# ---- with the evaluator and the genome archive --------------------------------------------------------------------------------

def test_chain_generate_evaluate():
    """generator3d_for(ev).generate -> ev.evaluate(levels, holes) on one stream, against evaluate on the twin's levels"""
    rng = np.random.default_rng(4480)
    G, S, shape = 4, 3, (5, 5, 5)
    for problem in ("dungeon", "maze"):
        with Mc3dHoleyEvaluator(problem, shape, device=DEV) as ev, generator3d_for(ev, n_steps=6) as gen:
            T = ev.spec.n_tiles
            assert (gen.n_tiles, gen.map_shape, gen.n_steps, gen.holey) == (T, shape, 6, True)
            assert (gen.border_tile, gen.empty_tile) == (1, 0) and gen.n_params == nca3d.n_params(T)
            w, init, holes = genomes(rng, G, T), seeds(rng, (S,), shape, T), some_holes(rng, shape, S)
            out = device_run(gen, w, init, holes, frames=False)
            per_level = _t(np.tile(holes, (G, 1, 1)))
            res = ev.evaluate(out.levels.view(G * S, *shape), per_level)
            want = nca3d.generated(w, init, holes, 6, n_tiles=T)
            same(out, want)
            assert len(np.unique(want.levels.reshape(G * S, -1), axis=0)) > 1
            ref = ev.evaluate(_t(want.levels.reshape((G * S,) + shape)), per_level)
            for key in ("stats", "loss", "play", "error"):
                assert torch.equal(res[key], ref[key]), (problem, key)
            gen.check_errors(), ev.check_errors()
    with pytest.raises(TypeError, match="generator3d_for"):
        generator3d_for(object())


def test_one_generation_with_the_holey_dungeon():
    """NcaEvolution.generation with Mc3dHoleyEvaluator (dungeon, 5 x 5 x 5, 8 children x 2 seeds): the children, levels,
    aggregate and archive equal the numpy twins (evo.gaussian_children, nca3d.generated, evo.aggregated, archive_rules)"""
    n, S, shape, n_steps, names = 8, 2, (5, 5, 5), 6, ["path-length", "n_jump"]
    rng = np.random.default_rng(4490)
    ev = Mc3dHoleyEvaluator("dungeon", shape, device=DEV)
    gen = generator3d_for(ev, n_steps=n_steps)
    T = ev.spec.n_tiles
    arc = genome_archive_for(ev, names, bins=4, n_params=gen.n_params)
    assert arc.n_params == gen.n_params == nca3d.n_params(T) and arc.dims == (4, 4)
    holes = some_holes(rng, shape, S)
    score = mc3d_holey_score(ev, names, _t(holes))
    init = seeds(rng, (S,), shape, T)
    mean = (rng.standard_normal(arc.n_params) * 0.2).astype(np.float32)
    evolution = NcaEvolution(gen, score, arc)
    ref = E.SeqGenomes(arc.dims, arc.bounds, arc.n_params)
    draw = 0
    for first, sigma in ((True, 0.3), (False, 0.1)):
        res = evolution.generation(_t(init), n, seed=3, sigma=sigma, first=first, mean=_t(mean) if first else None,
                                   holes=_t(holes))
        assert res.diversity_bonus is None  # there is no 3-D diversity kernel
        if first:
            parents, parent_cell = np.zeros((n, arc.n_params), np.float32) + mean, None
        else:
            occ = ref.occupied()
            parent_cell = occ[archive.sampled_parents(3, draw, n, len(occ))]
            parents = ref.maps.reshape(ref.cells, -1).view(np.float32)[parent_cell]
            assert np.array_equal(_np(res.parent_cell), parent_cell)
        kids = evo.gaussian_children(parents, 3, draw, sigma)
        draw += 1
        want = nca3d.generated(kids, init, holes, n_steps, n_tiles=T)
        assert E.same_bits(_np(res.genomes), kids)
        assert np.array_equal(_np(res.levels), want.levels) and np.array_equal(_np(res.n_step), want.n_step)
        objective, beh = score(_t(want.levels.reshape((n * S,) + shape)))
        agg = evo.aggregated(_np(objective).reshape(n, S), _np(beh).reshape(n, S, -1), want.n_step, weight=10.0)
        for name in ("behaviours", "objective", "variance_penalty"):
            assert E.same_bits(_np(getattr(res.aggregate, name)), getattr(agg, name)), name
        assert np.array_equal(_np(res.aggregate.time_penalty), agg.time_penalty)
        assert np.array_equal(_np(res.aggregate.valid), agg.valid) and agg.valid.all()
        status, cell, counts = ref.add_genomes(kids, agg.objective, agg.behaviours)
        assert np.array_equal(_np(res.added.status), status) and np.array_equal(_np(res.added.cell), cell)
        assert np.array_equal(_np(res.added.counts), counts)
        d = arc.dense()
        assert np.array_equal(_np(d.occupied), ref.flag) and np.array_equal(_np(d.grids), ref.maps)
        assert E.same_bits(_np(d.objectives), ref.obj) and E.same_bits(_np(d.behaviours), ref.beh)
        assert ref.flag.sum() >= 1
    arc.check_errors(), gen.check_errors(), ev.check_errors()
    arc.close(), gen.close(), ev.close()
