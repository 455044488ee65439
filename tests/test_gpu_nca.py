"""The NCA level generator on the device (include/pcgrl_amd_nca.h) against its numpy twins
(control_pcgrl_amd/nca.py): levels, n_step, frames and the error bits are equal bit for bit.  What runs: every tile count 2..8
(CASES has 2, 3 and 8; GEOMETRY all seven); blocks of 64 lanes (1 to 64 cells), 128 (65, 77, 128), 192 (129, 130, 192) and 256
(195, 256), and several passes of 256 lanes above 256 cells with a last pass of 1, 4 or 49 cells or a full one (260, 512, 513,
561, 4096); the recorded reference roll-outs (T = 2, 3, 8) and, for every tile count, the float64 statement of the step
(tests/nca_reference.py); the pick on exact logits (ties in the middle, in the denormal band, at 0 and at 1; the shortcut's
edges); a non-finite logit after valid steps; another stream; and the chains with the evaluators and the archive."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import archive_rules as AR
import ddave_rules as DR
import measures_numpy as mn
import nca_reference as nr
import pcgrl_oracle as po
from conftest import GOLDEN
from nca_reference import genomes, seeds
from control_pcgrl_amd import DDaveEvaluator, NcaGenerator, VecPcgrlEnv, archive, archive_for, generator_for, nca

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (map shape, T, n_steps, G, S, per-genome seeds)
CASES = [((1, 1), 2, 10, 3, 5, False), ((1, 9), 3, 2, 3, 5, True), ((9, 1), 8, 10, 3, 5, False), ((3, 3), 2, 1, 3, 5, True),
         ((5, 7), 3, 10, 3, 5, False), ((8, 8), 8, 10, 3, 5, True), ((10, 13), 2, 10, 3, 5, False), ((16, 16), 2, 10, 3, 5, True),
         ((16, 16), 8, 10, 3, 5, False), ((16, 16), 3, 2, 3, 5, True), ((17, 33), 3, 10, 2, 3, True),
         ((64, 64), 8, 2, 2, 2, False), ((64, 64), 2, 10, 1, 2, True)]


def _np(t):
    return t.cpu().numpy()


def device_run(gen, weights, init, n_steps=None, frames=True, out=None):
    return gen.generate(torch.as_tensor(weights).to(DEV), torch.as_tensor(init).to(DEV), n_steps=n_steps, frames=frames, out=out)


def same(out, want, what=""):
    assert np.array_equal(_np(out.n_step), want.n_step), (what, _np(out.n_step), want.n_step)
    assert np.array_equal(_np(out.levels), want.levels), what
    if out.frames is not None:
        assert np.array_equal(_np(out.frames), want.frames), what


@functools.lru_cache(maxsize=None)
def case(i):
    shape, T, n_steps, G, S, per = CASES[i]
    rng = np.random.default_rng(100 + i)
    w = genomes(rng, G, T)
    init = seeds(rng, (G, S) if per else (S,), shape, T)
    return w, init, nca.generated(w, init, n_steps, n_tiles=T)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{c[0][0]}x{c[0][1]}-T{c[1]}-n{c[2]}" for c in CASES])
def test_device_equals_twin(i):
    shape, T, n_steps, G, S, per = CASES[i]
    w, init, want = case(i)
    with NcaGenerator(T, shape, n_steps=n_steps, device=DEV) as gen:
        assert gen.n_params == w.shape[1]
        same(device_run(gen, w, init), want, CASES[i])
        bare = device_run(gen, w, init, frames=False)
        assert bare.frames is None
        same(bare, want, CASES[i])
        assert gen.poll_errors() == want.error_bits == 0
    assert (want.n_step >= 0).all()


def test_zero_weights():
    with NcaGenerator(2, (16, 16), device=DEV) as gen:
        zero = np.zeros((1, gen.n_params), np.float32)
        out = device_run(gen, zero, np.zeros((3, 16, 16), np.uint8))
        assert (_np(out.n_step) == 0).all() and (_np(out.levels) == 0).all() and (_np(out.frames) == 0).all()
        ones = np.ones((1, 16, 16), np.uint8)  # every sigmoid 0.5: the first index wins once, then the map stands
        out = device_run(gen, zero, ones)
        same(out, nca.generated(zero, ones, 10))
        assert _np(out.n_step).tolist() == [[1]]
        gen.check_errors()


def test_pairs_stop_at_different_steps():
    """the recorded genomes on their recorded seeds: clean and exempt trajectories, early and full-length ones, in one batch"""
    for path in sorted(glob.glob(os.path.join(GOLDEN, "nca", "*16x16.npz"))):
        z = np.load(path)
        T = int(z["n_tiles"])
        init = z["init"][:10]
        want = nca.generated(z["weights"], init, 10, n_tiles=T)
        assert len(np.unique(want.n_step)) > 1, np.unique(want.n_step)
        with generator_for(VecPcgrlEnv("binary" if T == 2 else "zelda", "narrow", (16, 16), 1, device=DEV)) as gen:
            assert (gen.n_tiles, gen.map_shape) == (T, (16, 16))
            same(device_run(gen, z["weights"], init), want, path)
            gen.check_errors()


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "nca", "*.npz"))), ids=os.path.basename)
def test_reference_fixtures_on_the_device(path):
    """every recorded step at every non-exempt cell (one step from the reference's own map: n_steps = 1), and the clean
    trajectories end to end"""
    z = np.load(path)
    T, n_steps = int(z["n_tiles"]), int(z["n_steps"])
    shape = z["init"].shape[1:]
    with NcaGenerator(T, shape, n_steps=n_steps, device=DEV) as gen:
        rows = np.flatnonzero(z["clean"])
        per_genome = z["weights"][z["genome"][rows]]  # one genome row per trajectory, its own seed
        out = device_run(gen, per_genome, z["init"][rows][:, None])
        assert np.array_equal(_np(out.n_step)[:, 0], z["n_step"][rows])
        assert np.array_equal(_np(out.frames)[:, 0], z["frames"][rows])
        assert np.array_equal(_np(out.levels)[:, 0], z["frames"][rows, -1])
        # single steps from the recorded maps
        prev = np.concatenate([z["init"][:, None], z["frames"][:, :-1]], axis=1)  # the map before step k
        live = np.arange(n_steps)[None, :] <= z["n_step"][:, None]
        idx = np.argwhere(live)
        one = device_run(gen, z["weights"][z["genome"][idx[:, 0]]], prev[idx[:, 0], idx[:, 1]][:, None], n_steps=1, frames=False)
        got = _np(one.levels)[:, 0]
        keep = ~z["exempt"][idx[:, 0], idx[:, 1]]
        assert keep.sum() > 0 and not (got != z["frames"][idx[:, 0], idx[:, 1]])[keep].any()
        gen.check_errors()


def test_saturated_ties():
    """genomes scaled by 50: logits in the hundreds, float32 sigmoids that tie at 1 (and at 0), the first index wins"""
    rng = np.random.default_rng(7)
    for T, shape in ((2, (16, 16)), (8, (16, 16)), (3, (5, 7))):
        w = genomes(rng, 3, T, scale=50.0)
        init = seeds(rng, (5,), shape, T)
        want = nca.generated(w, init, 10, n_tiles=T)
        _, logits = nca.stepped(nca.unpack_weights(w[0], T), init)
        s = nca.sigmoid32(logits)
        tied = (np.sort(s, axis=1)[:, -1] == np.sort(s, axis=1)[:, -2])
        assert tied.any() and (np.argmax(logits, axis=1) != np.argmax(s, axis=1)).any()  # an argmax over logits would differ
        with NcaGenerator(T, shape, device=DEV) as gen:
            same(device_run(gen, w, init), want, (T, shape))
            assert gen.poll_errors() == 0


def test_errors_leave_neighbours_alone():
    rng = np.random.default_rng(8)
    T, shape = 3, (16, 16)
    w = genomes(rng, 3, T)
    w[1, nca.n_params(T) - 2 * 32 - T + 5] = np.inf  # l3.weight[1, 5] of genome 1
    init = seeds(rng, (3, 4), shape, T)
    init[2, 1, 15, 15] = T  # a bad tile in the last cell of (genome 2, seed 1)
    init[0, 3, 0, 0] = 255
    want = nca.generated(w, init, 10, n_tiles=T)
    assert want.error_bits == (nca.ERR_TILE | nca.ERR_NONFINITE)
    assert want.n_step[1].tolist() == [-1] * 4 and want.n_step[2, 1] == -1 and want.n_step[0, 3] == -1
    assert (want.n_step >= 0).sum() == 6
    with NcaGenerator(T, shape, device=DEV) as gen:
        out = device_run(gen, w, init)
        same(out, want)
        assert np.array_equal(_np(out.levels)[1], init[1])
        with pytest.raises(ValueError, match="non-finite"):
            gen.check_errors()
        gen.check_errors()  # cleared
        # each bit on its own
        ok = genomes(rng, 1, T)
        device_run(gen, ok, init[2])
        assert gen.poll_errors() == nca.ERR_TILE
        device_run(gen, w[1:2], init[1])
        assert gen.poll_errors() == nca.ERR_NONFINITE
        nan = ok.copy()
        nan[0, 7] = np.nan  # a NaN in layer 1 reaches the logits
        out = device_run(gen, nan, init[1])
        same(out, nca.generated(nan, init[1], 10, n_tiles=T))
        assert gen.poll_errors() == nca.ERR_NONFINITE and (_np(out.n_step) == -1).all()


def test_out_reuse_and_argument_checks():
    rng = np.random.default_rng(9)
    T, shape = 2, (9, 9)
    with NcaGenerator(T, shape, n_steps=4, device=DEV) as gen:
        w, init = genomes(rng, 2, T), seeds(rng, (3,), shape, T)
        out = device_run(gen, w, init)
        ptrs = (out.levels.data_ptr(), out.n_step.data_ptr(), out.frames.data_ptr())
        w2, init2 = genomes(rng, 2, T), seeds(rng, (2, 3), shape, T)
        again = device_run(gen, w2, init2, out=out)
        assert again is out and ptrs == (out.levels.data_ptr(), out.n_step.data_ptr(), out.frames.data_ptr())
        same(out, nca.generated(w2, init2, 4, n_tiles=T))
        with pytest.raises(ValueError, match="out.levels"):
            device_run(gen, genomes(rng, 3, T), init, out=out)
        with pytest.raises(ValueError, match="1730"):
            device_run(gen, np.zeros((2, 1729), np.float32), init)
        with pytest.raises(ValueError, match="float32"):
            device_run(gen, np.zeros((2, 1730), np.float64), init)
        with pytest.raises(ValueError, match="init_states"):
            device_run(gen, w, seeds(rng, (3,), (9, 8), T))
        with pytest.raises(ValueError, match="n_steps"):
            device_run(gen, w, init, n_steps=1025)
        gen.check_errors()
    with pytest.raises(ValueError, match=r"\[2, 8\]"):
        NcaGenerator(9, (16, 16), device=DEV)
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        NcaGenerator(2, (65, 16), device=DEV)
    with pytest.raises(RuntimeError, match="closed"):
        gen.generate(torch.zeros((1, 1730), device=DEV), torch.zeros((1, 9, 9), dtype=torch.uint8, device=DEV))


def test_long_rollout():
    """n_steps far past the reference's 10: the loop, the frame rows and the early stop are the same code"""
    rng = np.random.default_rng(10)
    T, shape = 2, (5, 7)
    w, init = genomes(rng, 2, T), seeds(rng, (2,), shape, T)
    want = nca.generated(w, init, 64, n_tiles=T)
    with NcaGenerator(T, shape, n_steps=64, device=DEV) as gen:
        same(device_run(gen, w, init), want)


def test_captured_graph_replays_on_new_inputs():
    rng = np.random.default_rng(11)
    T, shape, G, S = 2, (16, 16), 4, 3
    with NcaGenerator(T, shape, device=DEV) as gen:
        w = torch.as_tensor(genomes(rng, G, T)).to(DEV)
        init = torch.as_tensor(seeds(rng, (S,), shape, T)).to(DEV)
        out = gen.generate(w, init, frames=True)  # eager once
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            gen.generate(w, init, frames=True, out=out)
        for replay in range(2):
            w2, i2 = genomes(rng, G, T), seeds(rng, (S,), shape, T)
            w.copy_(torch.as_tensor(w2)), init.copy_(torch.as_tensor(i2))
            graph.replay()
            torch.cuda.synchronize()
            same(out, nca.generated(w2, i2, 10, n_tiles=T), replay)
        gen.check_errors()


def test_chain_generate_stats_measures():
    """generate -> stats_for_grids -> measures on binary 16 x 16, one stream, no host sync in between, against the twin's maps
    through the CPU oracle and the numpy measures"""
    rng = np.random.default_rng(12)
    G, S = 6, 5
    env = VecPcgrlEnv("binary", "narrow", (16, 16), 1, device=DEV)
    with generator_for(env) as gen:
        w, init = genomes(rng, G, 2), seeds(rng, (S,), (16, 16), 2)
        out = device_run(gen, w, init, frames=False)
        stats = env.stats_for_grids(out.levels)
        m = env.measures_for_grids(out.levels)
        want = nca.generated(w, init, 10, n_tiles=2)
        maps = want.levels.reshape(G * S, 16, 16)
        assert np.array_equal(_np(out.levels).reshape(G * S, 16, 16), maps)
        assert np.array_equal(_np(stats), po.stats_for_grids("binary", maps))
        assert np.array_equal(_np(m.counts), mn.counts(maps, 2)) and np.array_equal(_np(m.match), mn.matches(maps, 2))
        assert len(np.unique(maps.reshape(G * S, -1), axis=0)) > 1
        gen.check_errors()
        env.check_errors()
    env.close()


# ---- every tile count, block size and last pass -------------------------------------------------------------------------------

# map shape -> the tile counts run on it: every T at 7 x 11 (128 lanes, Dave's stock map) and 13 x 20 (a second pass of four
# cells) and on one more shape; every shape with two tile counts, one of them with a padded w3t row (5, 6, 7)
GEOMETRY = {(7, 9): (5, 2),                # 63 cells: 64 lanes
            (5, 13): (6, 3),               # 65: 128 lanes
            (7, 11): (2, 3, 4, 5, 6, 7, 8),  # 77: 128 lanes
            (8, 16): (7, 4),               # 128: 128 lanes, full
            (3, 43): (5, 8),               # 129: 192 lanes
            (12, 16): (6, 2),              # 192: 192 lanes, full
            (13, 15): (7, 3),              # 195: 256 lanes
            (13, 20): (2, 3, 4, 5, 6, 7, 8),  # 260: a second pass of 4 cells
            (8, 64): (5, 4),               # 512: two full passes
            (19, 27): (6, 8)}              # 513: a third pass of one cell
GEOMETRY_CASES = [(shape, T) for shape, tiles in GEOMETRY.items() for T in tiles]
EXEMPT_CAP = 0.02  # as tests/test_nca_cpu.py


@pytest.mark.parametrize("n", range(len(GEOMETRY_CASES)), ids=[f"{s[0]}x{s[1]}-T{T}" for s, T in GEOMETRY_CASES])
def test_every_tile_count_and_block_size(n):
    shape, T = GEOMETRY_CASES[n]
    G, S, n_steps, per = 2, 3, 4, bool(n % 2)
    rng = np.random.default_rng(3850 + n)
    w = genomes(rng, G, T)
    init = seeds(rng, (G, S) if per else (S,), shape, T)
    want = nca.generated(w, init, n_steps, n_tiles=T)
    with NcaGenerator(T, shape, n_steps=n_steps, device=DEV) as gen:
        same(device_run(gen, w, init), want, (shape, T))
        bare = device_run(gen, w, init, frames=False)
        assert bare.frames is None
        same(bare, want, (shape, T))
        # the single steps of the twin's trajectory against the float64 statement of the step
        first = np.broadcast_to(init, (G,) + init.shape[-3:])
        prev = np.concatenate([first[:, :, None], want.frames[:, :, :-1]], axis=2)  # the map before step k
        idx = np.argwhere(np.arange(n_steps)[None, None, :] <= want.n_step[:, :, None])
        maps = prev[idx[:, 0], idx[:, 1], idx[:, 2]]
        one = device_run(gen, w[idx[:, 0]], maps[:, None], n_steps=1, frames=False)
        got = _np(one.levels)[:, 0]
        l64 = np.stack([nr.logits64(w[g], m, T) for g, m in zip(idx[:, 0], maps)])
        ex = nr.exempt(l64)
        print(f"{shape} T = {T}: exempt share {ex.mean():.5f} of {ex.size} cells")
        assert ex.mean() <= EXEMPT_CAP and not (got != np.argmax(l64, axis=-3))[~ex].any()
        assert np.array_equal(got, want.frames[idx[:, 0], idx[:, 1], idx[:, 2]])
        assert gen.poll_errors() == want.error_bits == 0


# ---- the pick on exact logits -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", range(2, 9))
def test_pick_on_exact_logits(T):
    """a genome that is zero but for l3.bias has exactly that vector as every cell's logits (a -0.0 becomes +0.0 when the
    zero products are added): one genome on a 1 x 1 map is one probe of the pick, the whole probe set one launch"""
    p = nr.probe_vectors(T, np.random.default_rng(380 + T))
    w = nr.bias_genomes(p.vectors, T)
    assert len(w) <= (3000 if T <= 4 else 2000) and w.nbytes < 30e6
    init = np.zeros((1, 1, 1), np.uint8)
    for g in range(0, len(w), 97):
        _, logits = nca.stepped(w[g], init[0], n_tiles=T)
        assert np.array_equal(logits[:, 0, 0], p.vectors[g])
    twin = np.argmax(nca.sigmoid32(p.vectors), axis=-1)
    ref, gap = nr.pick_ref(p.vectors)
    keep = gap >= nr.GAP_FLOOR
    with NcaGenerator(T, (1, 1), n_steps=1, device=DEV) as gen:
        out = device_run(gen, w, init, frames=False)
        got = _np(out.levels)[:, 0, 0, 0]
        bad = np.flatnonzero(got != twin)
        assert bad.size == 0, [(int(i), str(p.family[i]), p.vectors[i].tolist(), int(got[i]), int(twin[i])) for i in bad[:8]]
        assert (~keep).sum() <= 0.001 * len(keep) and np.array_equal(got[keep], ref[keep])
        assert (_np(out.n_step) == 0).all()
        assert gen.poll_errors() == 0


# ---- a non-finite logit after valid steps -------------------------------------------------------------------------------------

def overflow_genome(T=4):
    """Reads centre taps only.  A cell of tile 1 becomes 2 (unit 3 carries 2 to logit 2), a cell of tile 2 becomes 3 (unit 4),
    a cell of tile 0 stays (all logits equal: the first index).  At a cell of tile 3 units 0 and 1 are 3e38 each and layer 2
    adds them: inf, and 0 * inf in layer 3 -- a NaN in every logit of that one cell."""
    g = np.zeros(nca.n_params(T), np.float32)
    w = nca.unpack_weights(g, T)
    w.w1[3, 1, 1, 1] = w.w2[3, 3] = w.w1[4, 2, 1, 1] = w.w2[4, 4] = 1.0
    w.w3[2, 3] = w.w3[3, 4] = 2.0
    w.w1[0, 3, 1, 1] = w.w1[1, 3, 1, 1] = 3e38
    w.w2[0, 0] = w.w2[0, 1] = 1.0
    return g


def first_nonfinite(w, init, T, n_steps):
    """the twin's first step with a non-finite logit on one map, or None"""
    cur = init
    for step in range(n_steps):
        nxt, logits = nca.stepped(w, cur, n_tiles=T)
        if not np.isfinite(logits).all():
            return step
        if (nxt == cur).all():
            return None
        cur = nxt
    return None


@pytest.mark.parametrize("shape", [(16, 16), (17, 33)], ids=["16x16", "17x33"])
def test_nonfinite_after_the_first_step(shape):
    """the refusal overwrites the frame rows that valid steps wrote, also where a lane owns several cells (17 x 33: three
    passes; the cell that overflows is in the last pass, in the second, or is cell 0)"""
    T, n_steps, rng = 4, 6, np.random.default_rng(3860)
    H, W = shape
    w = genomes(rng, 3, T)
    w[1] = overflow_genome(T)
    init = seeds(rng, (3, 4), shape, T)
    init[1] = 0
    init[1, 0, H - 1, W - 1] = 1   # 1 -> 2 -> 3 -> overflow at step 2, in the last cell
    init[1, 1, H // 2, 3] = 2      # 2 -> 3 -> overflow at step 1, mid-map
    init[1, 2, 0, 0] = 2           # the same in cell 0, with a tile 1 that is still on its way
    init[1, 2, H - 1, 0] = 1
    assert first_nonfinite(w[1], init[1, 0], T, n_steps) == 2 and first_nonfinite(w[1], init[1, 1], T, n_steps) == 1
    assert first_nonfinite(w[1], init[1, 2], T, n_steps) == 1 and first_nonfinite(w[1], init[1, 3], T, n_steps) is None
    want = nca.generated(w, init, n_steps, n_tiles=T)
    assert want.error_bits == nca.ERR_NONFINITE and want.n_step[1].tolist() == [-1, -1, -1, 0]
    assert (want.n_step[[0, 2]] >= 0).all() and (want.frames[1, :3] == init[1, :3, None]).all()
    with NcaGenerator(T, shape, n_steps=n_steps, device=DEV) as gen:
        out = device_run(gen, w, init)
        same(out, want, shape)
        assert np.array_equal(_np(out.levels)[1], init[1]) and (_np(out.frames)[1] == init[1][:, None]).all()
        assert gen.poll_errors() == nca.ERR_NONFINITE and gen.poll_errors() == 0
        same(device_run(gen, w, init, frames=False), want, shape)
        assert gen.poll_errors() == nca.ERR_NONFINITE and gen.poll_errors() == 0


# ---- with the Dave evaluator and the archive; another stream ------------------------------------------------------------------

def test_generation_with_the_dave_evaluator():
    """generate -> evaluate -> behaviour -> archive add -> ask on one stream with no host sync in between: T = 7 on Dave's
    7 x 11 map (128 lanes), against the twin's maps through tests/ddave_rules.py, the numpy measures and
    tests/archive_rules.py"""
    rng = np.random.default_rng(3870)
    G, S, T, names = 6, 4, 7, ["emptiness", "symmetry"]
    ev = DDaveEvaluator((7, 11), DEV, solver_power=200, max_levels=64)
    gen, arc = generator_for(ev), archive_for(ev, names, bins=10)
    assert (gen.n_tiles, gen.map_shape, gen.n_params) == (T, (7, 11), nca.n_params(T))
    w, init = genomes(rng, G, T), seeds(rng, (S,), (7, 11), T)
    out = device_run(gen, w, init, frames=False)
    levels = out.levels.reshape(G * S, 7, 11)
    res = ev.evaluate(levels)
    objective = ev.reward(res["stats"], torch.zeros_like(res["stats"]))
    beh = ev.behaviour(levels, names)
    added = arc.add(levels, objective, beh)
    kids, parent = arc.ask(16, seed=5, rate=0.05)
    # everything above is enqueued; from here on the host reads
    want = nca.generated(w, init, 10, n_tiles=T)
    same(out, want)
    maps = want.levels.reshape(G * S, 7, 11)
    assert len(np.unique(maps.reshape(G * S, -1), axis=0)) > 1
    rows = [DR.outputs(m, 200, 0) for m in maps]
    stats = np.asarray([r[0] for r in rows], np.int32)
    assert np.array_equal(_np(res["stats"]), stats)
    assert np.array_equal(_np(res["play"]), np.asarray([r[3] for r in rows], np.int32))
    want_obj = np.array([DR.reward(s, [0] * 11) for s in stats], np.float64)
    assert np.array_equal(_np(objective).view(np.uint64), want_obj.view(np.uint64))
    bc = mn.bc_from_integers(mn.counts(maps, T), mn.matches(maps, T), 7, 11, T)
    want_beh = np.stack([bc[k] for k in names], 1)
    assert np.array_equal(_np(beh).view(np.uint64), want_beh.view(np.uint64))
    ref = AR.SeqArchive(arc.dims, arc.bounds, (7, 11))
    status, cell, counts = ref.add(maps, want_obj, want_beh)
    assert np.array_equal(_np(added.status), status) and np.array_equal(_np(added.cell), cell)
    assert np.array_equal(_np(added.counts), counts) and counts[0] >= 1 and counts[2] == 0
    d = arc.dense()
    assert np.array_equal(_np(d.occupied), ref.flag) and np.array_equal(_np(d.grids), ref.maps)
    assert np.array_equal(_np(d.objectives).view(np.uint64), ref.obj.view(np.uint64))
    occ = ref.occupied()
    pc = occ[archive.sampled_parents(5, 0, 16, len(occ))]
    assert np.array_equal(_np(parent), pc) and np.array_equal(_np(kids), archive.mutated(ref.maps[pc], 5, 0, 0.05, T))
    gen.check_errors(), ev.check_errors(), arc.check_errors()
    gen.close(), arc.close(), ev.close()
    # and generator_for on an env with five tiles
    env = VecPcgrlEnv("sokoban", "narrow", (8, 8), 1, device=DEV)
    with generator_for(env, n_steps=5) as gen:
        assert (gen.n_tiles, gen.map_shape, gen.n_steps) == (5, (8, 8), 5)
        w, init = genomes(rng, 3, 5), seeds(rng, (3, 2), (8, 8), 5)
        same(device_run(gen, w, init), nca.generated(w, init, 5, n_tiles=5))
        gen.check_errors()
    env.close()


def test_side_stream_and_second_run_are_byte_identical():
    rng = np.random.default_rng(3880)
    T, shape, G, S = 6, (7, 11), 4, 3
    with NcaGenerator(T, shape, n_steps=8, device=DEV) as gen:
        w = torch.as_tensor(genomes(rng, G, T)).to(DEV)
        init = torch.as_tensor(seeds(rng, (G, S), shape, T)).to(DEV)
        first = gen.generate(w, init, frames=True)
        second = gen.generate(w, init, frames=True)
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            third = gen.generate(w, init, frames=True)
            assert gen.poll_errors() == 0  # (synchronises the side stream)
        torch.cuda.current_stream(DEV).wait_stream(side)
        for other in (second, third):
            for name in ("levels", "n_step", "frames"):
                assert getattr(other, name).data_ptr() != getattr(first, name).data_ptr()
                assert torch.equal(getattr(other, name), getattr(first, name)), name
        same(first, nca.generated(_np(w), _np(init), 8, n_tiles=T))
        assert gen.poll_errors() == 0
