"""NCA evolution on the device against its numpy twins, bit for bit (include/pcgrl_amd_evo.h): Gaussian
children and samples, genome payloads through add / elites / stats / the image against archive_rules' insertion, the fold over
seeds, and whole generations -- uncaptured and in one graph -- against the composed chain of twins."""
import math

import numpy as np
import pytest
import torch

import evo_rules as E
from control_pcgrl_amd import (DDaveEvaluator, DeviceGridArchive, GenomeArchive, LodeRunnerEvaluator, NcaEvolution, archive, evo,
                               evaluator_score, generator_for, genome_archive_for, nca)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUNDS = [(0.0, 1.0), (-2.5, 7.0)]


def _np(t):
    return t.cpu().numpy()


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a) if dtype is None else np.asarray(a, dtype)).to(DEV)


def pair(dims, bounds, P):
    return GenomeArchive(dims, bounds, P, device=DEV), E.SeqGenomes(dims, bounds, P)


def same(arc, ref, what=""):
    """the whole device archive against the restatement: flags, objectives, behaviours, payload rows, stats() and elites()"""
    d = arc.dense()
    assert np.array_equal(_np(d.occupied), ref.flag), what
    assert E.same_bits(_np(d.objectives), ref.obj) and E.same_bits(_np(d.behaviours), ref.beh), what
    assert np.array_equal(_np(d.grids), ref.maps), what
    occ, st = ref.occupied(), arc.stats()
    assert st.count == len(occ), what
    if len(occ):
        o = ref.obj[occ]
        assert st.max == o.max() and st.min == o.min(), what
    el = arc.elites()
    assert np.array_equal(_np(el.cells), occ) and E.same_bits(_np(el.objectives), ref.obj[occ]), what
    assert E.same_bits(_np(el.behaviours), ref.beh[occ]), what
    assert el.genomes.dtype == torch.float32 and tuple(el.genomes.shape) == (len(occ), arc.n_params), what
    assert np.array_equal(_np(el.genomes).view(np.uint8), ref.maps[occ]), what


def add_both(arc, ref, genomes, obj, beh=None, cells=None, what="", refused=False):
    out = arc.add(_t(genomes, np.float32), _t(obj, np.float64), None if beh is None else _t(beh, np.float64),
                  None if cells is None else _t(cells, np.int32))
    status, cell, counts = ref.add_genomes(genomes, np.asarray(obj, np.float64), beh, cells)
    assert np.array_equal(_np(out.status), status), (what, _np(out.status), status)
    assert np.array_equal(_np(out.cell), cell) and np.array_equal(_np(out.counts), counts), what
    if refused:
        assert (status == 3).any()
        with pytest.raises(ValueError, match="refused"):
            arc.check_errors()
    arc.check_errors()
    same(arc, ref, what)


def _genomes(rng, n, P):
    return (rng.standard_normal((n, P)) * 0.3).astype(np.float32)


def _fill(arc, ref, rng, k):
    """k occupied cells of a (3, 4) archive"""
    cells = rng.permutation(12)[:k]
    add_both(arc, ref, _genomes(rng, k, arc.n_params), rng.random(k), cells=cells, what=f"fill {k}")


# ---- ask_genomes and sample_genomes -----------------------------------------------------------------------------------------

def _offset_out(n, P, off_bytes):
    buf = torch.full((n * P + 8,), 7.25, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    k = (off_bytes // 4) % 4
    out = buf[k:k + n * P].view(n, P)
    assert out.data_ptr() % 16 == off_bytes % 16
    return buf, out, k


@pytest.mark.parametrize("P", [1, 3, 4, 5, 63, 64, 65, 1730, 3656, 16384])
def test_ask_genomes_equals_the_twins(P):
    rng = np.random.default_rng(P)
    # (occupied cells, [(n, sigma, byte offset of out), ...]): two calls in a row use draws d and d + 1
    plan = [(1, [(1, 0.0, 4), (300, 0.1, 8)]), (2, [(2, 1e-30, 12), (65, 3e38, 0)]), (12, [(65, 0.1, 4), (2, 0.0, 12), (1, 3e38, 8)])]
    for k, calls in plan:
        arc, ref = pair((3, 4), BOUNDS, P)
        _fill(arc, ref, rng, k)
        occ = ref.occupied()
        rows = ref.maps.reshape(12, -1).view(np.float32)
        for draw, (n, sigma, off) in enumerate(calls):
            buf, out, at = _offset_out(n, P, off)
            kids, parent = arc.ask(n, seed=11 + P, sigma=sigma, out=out)
            assert kids is out
            p = occ[archive.sampled_parents(11 + P, draw, n, k)]
            assert np.array_equal(_np(parent), p), (k, draw)
            want = evo.gaussian_children(rows[p], 11 + P, draw, sigma)
            got = _np(kids)
            assert E.same_bits(got, want), (k, draw, n, sigma)
            assert not np.isnan(got).any()
            if sigma == 0.0:
                assert E.same_bits(got, rows[p])  # the parents' bits
            elif sigma > 1e38:  # the overflow case: inf where |z| sigma passes float32, and only inf
                assert np.isinf(got).any() or n * P < 64
            else:
                assert np.isfinite(got).all() and (sigma < 0.1 or n * P < 4 or not np.array_equal(got, rows[p]))
            edge = _np(buf)
            assert (edge[:at] == 7.25).all() and (edge[at + n * P:] == 7.25).all()  # nothing outside the rows
        arc.check_errors()
        same(arc, ref, "asking changes nothing")
        arc.close()


def test_sample_genomes_and_the_empty_archive():
    P, n = 1730, 65
    arc, ref = pair((3, 4), BOUNDS, P)
    out = torch.full((n, P), -3.0, dtype=torch.float32, device=DEV)
    parent = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    arc.ask(n, seed=1, out=(out, parent))
    with pytest.raises(RuntimeError, match="empty archive"):
        arc.check_errors()
    assert (out == -3.0).all().item() and (parent == -7).all().item()
    # the refused ask drew nothing: the first sample is draw 0, the next draw 1, with and without a mean
    zero = np.zeros((n, P), np.float32)
    got = arc.sample(n, seed=5, sigma=0.1)
    assert E.same_bits(_np(got), evo.gaussian_children(zero, 5, 0, 0.1))
    mean = _genomes(np.random.default_rng(0), 1, P)[0]
    got = arc.sample(n, seed=5, sigma=0.25, mean=_t(mean), out=out)
    assert got is out and E.same_bits(_np(got), evo.gaussian_children(zero + mean, 5, 1, 0.25))
    assert E.same_bits(_np(arc.sample(3, seed=5, sigma=0.0, mean=_t(mean))), zero[:3] + mean)  # draw 2
    assert arc.stats().count == 0
    # the counter is shared with ask: the next ask is draw 3
    rng = np.random.default_rng(1)
    _fill(arc, ref, rng, 5)
    kids, parent = arc.ask(n, seed=5, sigma=0.1)
    p = ref.occupied()[archive.sampled_parents(5, 3, n, 5)]
    assert np.array_equal(_np(parent), p)
    assert E.same_bits(_np(kids), evo.gaussian_children(ref.maps.reshape(12, -1).view(np.float32)[p], 5, 3, 0.1))
    arc.check_errors()
    for bad in (-0.1, math.inf, math.nan):
        with pytest.raises(ValueError, match="sigma"):
            arc.ask(2, sigma=bad)
        with pytest.raises(ValueError, match="sigma"):
            arc.sample(2, sigma=bad)
    arc.close()


# ---- add / elites / stats on genome payloads -----------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 5, 3656])
@pytest.mark.parametrize("dims", [(1,), (3, 4), (64, 64)])
def test_genome_payloads_through_add(dims, P):
    rng = np.random.default_rng(100 * len(dims) + P)
    bounds = BOUNDS[:len(dims)]
    arc, ref = pair(dims, bounds, P)
    cells = int(np.prod(dims))
    special = np.array([0.0, -0.0, 1.0, 1.0, 2.0, -math.inf, math.inf])
    for n in (1, 64, 65, 1000):
        beh = np.stack([rng.uniform(lo - 0.1, hi + 0.1, n) for lo, hi in bounds], 1)
        obj = np.where(rng.random(n) < 0.5, rng.integers(0, 3, n).astype(np.float64), special[rng.integers(0, len(special), n)])
        add_both(arc, ref, _genomes(rng, n, P), obj, beh, what=f"n {n}")
    # refusals: a NaN objective, a NaN behaviour, and cells= with an index out of range
    n = 65
    beh = np.stack([rng.uniform(lo, hi, n) for lo, hi in bounds], 1)
    obj = rng.integers(0, 5, n).astype(np.float64)
    obj[3], beh[64, 0] = math.nan, math.nan
    add_both(arc, ref, _genomes(rng, n, P), obj, beh, what="NaN", refused=True)
    pick = rng.integers(0, cells, n)
    pick[7] = cells
    add_both(arc, ref, _genomes(rng, n, P), rng.integers(3, 9, n).astype(np.float64), cells=pick, what="cells=", refused=True)
    assert tuple(arc.cell_of(_t(beh)).shape) == (n,) and np.array_equal(_np(arc.cell_of(_t(beh))), archive.placed_cells(beh, dims, bounds))
    # rows at a 4-byte offset from a 16-byte boundary are copied whole
    buf = torch.as_tensor(_genomes(rng, 1, 4 * P + 1)[0]).to(DEV)
    g = buf[1:].view(4, P)
    out = arc.add(g, _t([50.0, 51.0, 52.0, 53.0]), cells=_t([0, 0, cells - 1, cells - 1], np.int32))
    status, cell, counts = ref.add_genomes(_np(g), np.array([50.0, 51.0, 52.0, 53.0]), None, [0, 0, cells - 1, cells - 1])
    assert np.array_equal(_np(out.status), status) and np.array_equal(_np(out.counts), counts)
    same(arc, ref, "offset rows")
    arc.close()


# ---- the image ---------------------------------------------------------------------------------------------------------------

def test_image_round_trip_and_refusals():
    rng = np.random.default_rng(8)
    P = 77
    arc, ref = pair((3, 4), BOUNDS, P)
    _fill(arc, ref, rng, 7)
    arc.ask(5, seed=2)
    arc.ask(5, seed=2)  # the counter is 2
    state = arc.state_dict()
    assert E.same_bits(_np(state["image"]), _np(arc.state_dict()["image"]))  # reproducible
    header = _np(state["image"][:48]).view(np.int32)
    assert header[7] == 4 * P and header[8] == 0  # L = 4 P, T = 0
    other, _ = pair((3, 4), BOUNDS, P)
    other.load_state_dict(state)
    same(other, ref, "restored")
    a, b = arc.ask(9, seed=2, sigma=0.2), other.ask(9, seed=2, sigma=0.2)  # both at draw 2
    assert E.same_bits(_np(a[0]), _np(b[0])) and np.array_equal(_np(a[1]), _np(b[1]))
    p = ref.occupied()[archive.sampled_parents(2, 2, 9, 7)]
    assert np.array_equal(_np(a[1]), p)
    assert E.same_bits(_np(other.state_dict()["image"]), _np(arc.state_dict()["image"]))
    # refusals, before anything is overwritten
    maps = DeviceGridArchive((3, 4), BOUNDS, (4 * P,), 8, device=DEV)  # a map archive whose rows are as long
    before = _np(maps.state_dict()["image"])
    with pytest.raises(ValueError, match="genome archive's image does not fit a map archive"):
        maps.load_state_dict(state)
    assert np.array_equal(_np(maps.state_dict()["image"]), before)
    with pytest.raises(ValueError, match="map archive's image does not fit a genome archive"):
        other.load_state_dict(maps.state_dict())
    for wrong, why in ((GenomeArchive((3, 4), BOUNDS, P + 1, device=DEV), "genome length"),
                       (GenomeArchive((4, 3), BOUNDS, P, device=DEV), "other dims")):
        with pytest.raises(ValueError, match=why):
            wrong.load_state_dict(state)
        assert wrong.stats().count == 0
        wrong.close()
    same(other, ref, "after the refusals")
    # each kind names the other's call
    with pytest.raises(ValueError, match="pcgrl_archive_ask_genomes"):
        DeviceGridArchive.ask(arc, 3)
    wrapped = GenomeArchive.__new__(GenomeArchive)  # the map archive's handle behind the genome calls
    wrapped.__dict__.update(maps.__dict__, n_params=P)
    with pytest.raises(ValueError, match="use pcgrl_archive_ask "):
        wrapped.ask(3)
    with pytest.raises(ValueError, match="use pcgrl_archive_ask "):
        wrapped.sample(3)
    wrapped._h = None  # (maps owns the handle)
    # a map archive's image is what it was: header L, T, and the sections' size
    assert _np(maps.state_dict()["image"][:48]).view(np.int32)[7:10].tolist() == [4 * P, 8, 0]
    arc.close(), other.close(), maps.close()


# ---- aggregate ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 3, 65])
def test_aggregate_equals_the_twin(G):
    side = torch.cuda.Stream(device=DEV)
    for S in E.S_GPU:
        for D in (1, 2, 3, 4):
            obj, beh, ns = E.aggregate_data(G, S, D, seed=G * 1000 + S * 10 + D)
            if G > 1:
                ns[G // 2, S // 2] = -1
            want = evo.aggregated(obj, beh, ns, weight=10.0)
            mean, o, tp, var, valid = E.numpy_fold(obj, beh, ns, 10.0)  # and numpy itself
            t = (_t(obj), _t(beh), _t(ns))
            if D == 2:
                side.wait_stream(torch.cuda.current_stream(DEV))
                with torch.cuda.stream(side):
                    got = evo.aggregate(*t, weight=10.0)
                side.synchronize()
            else:
                got = evo.aggregate(*t, weight=10.0)
            for name, arbiter in (("behaviours", mean), ("objective", o), ("variance_penalty", var)):
                assert E.same_bits(_np(getattr(got, name)), getattr(want, name)), (name, S, D)
                assert E.same_bits(_np(getattr(got, name)), arbiter), (name, S, D)
            assert np.array_equal(_np(got.time_penalty), tp) and np.array_equal(_np(got.valid), valid), (S, D)
            assert got.time_penalty.dtype == torch.int32 and got.valid.dtype == torch.uint8
    out = evo.aggregate(*t, weight=2.0)
    again = evo.aggregate(*t, weight=2.0, out=out)
    assert again is out
    with pytest.raises(ValueError, match=r"\[1, 128\]"):
        evo.aggregate(torch.zeros((1, 129), dtype=torch.float64, device=DEV), torch.zeros((1, 129, 1), dtype=torch.float64, device=DEV),
                      torch.zeros((1, 129), dtype=torch.int32, device=DEV))


# ---- whole generations --------------------------------------------------------------------------------------------------------

def _problem(kind):
    """the evaluator, the behaviour names and the score: evaluator_score for Lode Runner; Dangerous Dave has no loss, so its
    score is written here (the length of the solver's route as the objective)"""
    if kind == "loderunner":
        ev, names = LodeRunnerEvaluator((5, 7), device=DEV), ["emptiness", "path-length"]
        return ev, names, evaluator_score(ev, names, gold_cap=0)
    ev, names = DDaveEvaluator((7, 11), device=DEV), ["entropy", "co-occurance"]
    with pytest.raises(TypeError, match="no loss"):
        evaluator_score(ev, names)(torch.zeros((1, 7, 11), dtype=torch.uint8, device=DEV))

    def score(levels):
        return ev.evaluate(levels)["length"].to(torch.float64), ev.behaviour(levels, names)

    score.evaluator = ev
    return ev, names, score


class TwinChain:
    """the composed chain of twins: gaussian_children -> nca.generated -> the device evaluator's own outputs on those levels
    -> aggregated -> archive_rules"""

    def __init__(self, ev, score, arc, init, n_steps):
        self.ev, self.score, self.init, self.n_steps = ev, score, init, n_steps
        self.ref = E.SeqGenomes(arc.dims, arc.bounds, arc.n_params)
        self.P, self.T, self.draw = arc.n_params, ev.spec.n_tiles, 0

    def generation(self, n, seed, sigma, first=False, mean=None):
        if first:
            parents = np.zeros((n, self.P), np.float32) + (0 if mean is None else mean)
            parent_cell = None
        else:
            occ = self.ref.occupied()
            parent_cell = occ[archive.sampled_parents(seed, self.draw, n, len(occ))]
            parents = self.ref.maps.reshape(self.ref.cells, -1).view(np.float32)[parent_cell]
        kids = evo.gaussian_children(parents, seed, self.draw, sigma)
        self.draw += 1
        gen = nca.generated(kids, self.init, n_steps=self.n_steps, n_tiles=self.T)
        S = self.init.shape[0]
        levels = _t(gen.levels.reshape((n * S,) + gen.levels.shape[2:]))
        objective, beh = self.score(levels)
        agg = evo.aggregated(_np(objective).reshape(n, S), _np(beh).reshape(n, S, -1), gen.n_step, weight=10.0)
        status, cell, counts = self.ref.add_genomes(kids, agg.objective, agg.behaviours)
        return kids, parent_cell, gen, agg, status, cell, counts


def _check_generation(res, want, S):
    kids, parent_cell, gen, agg, status, cell, counts = want
    assert E.same_bits(_np(res.genomes), kids)
    assert (res.parent_cell is None) == (parent_cell is None)
    if parent_cell is not None:
        assert np.array_equal(_np(res.parent_cell), parent_cell)
    assert np.array_equal(_np(res.levels), gen.levels) and np.array_equal(_np(res.n_step), gen.n_step)
    for name in ("behaviours", "objective", "variance_penalty"):
        assert E.same_bits(_np(getattr(res.aggregate, name)), getattr(agg, name)), name
    assert np.array_equal(_np(res.aggregate.time_penalty), agg.time_penalty) and np.array_equal(_np(res.aggregate.valid), agg.valid)
    assert np.array_equal(_np(res.added.status), status) and np.array_equal(_np(res.added.cell), cell)
    assert np.array_equal(_np(res.added.counts), counts)
    if S > 1:
        assert tuple(res.diversity_bonus.shape) == (len(kids),)


def _setup(kind, S, bins=4, n_steps=6):
    ev, names, score = _problem(kind)
    arc = genome_archive_for(ev, names, bins=bins)
    gen = generator_for(ev, n_steps=n_steps)
    assert arc.n_params == gen.n_params == nca.n_params(ev.spec.n_tiles) and arc.dims == (bins, bins)
    rng = np.random.default_rng(31)
    init = rng.integers(0, ev.spec.n_tiles, (S,) + tuple(ev.map_shape), dtype=np.uint8)
    mean = (rng.standard_normal(arc.n_params) * 0.4).astype(np.float32)
    return ev, names, score, arc, gen, init, mean


@pytest.mark.parametrize("kind,G,S", [("loderunner", 6, 3), ("ddave", 5, 2)])
def test_generations_equal_the_composed_chain(kind, G, S):
    ev, names, score, arc, gen, init, mean = _setup(kind, S)
    evolution = NcaEvolution(gen, score, arc)
    chain = TwinChain(ev, score, arc, init, gen.n_steps)
    d_init, d_mean = _t(init), _t(mean)
    res = evolution.generation(d_init, G, seed=3, sigma=0.3, first=True, mean=d_mean)
    _check_generation(res, chain.generation(G, 3, 0.3, first=True, mean=mean), S)
    same(arc, chain.ref, "the first generation")
    assert chain.ref.flag.sum() >= 1
    for g in range(2):
        res = evolution.generation(d_init, G, seed=3, sigma=0.1)
        _check_generation(res, chain.generation(G, 3, 0.1), S)
        same(arc, chain.ref, f"generation {g + 1}")
    arc.check_errors(), gen.check_errors(), ev.check_errors()
    arc.close(), gen.close(), ev.close()


def test_a_generation_in_one_graph():
    G, S = 6, 3
    ev, names, score, arc, gen, init, mean = _setup("loderunner", S)
    evolution = NcaEvolution(gen, score, arc)
    chain = TwinChain(ev, score, arc, init, gen.n_steps)
    d_init, d_mean = _t(init), _t(mean)
    evolution.generation(d_init, G, seed=3, sigma=0.3, first=True, mean=d_mean)  # draw 0
    chain.generation(G, 3, 0.3, first=True, mean=mean)
    evolution.generation(d_init, G, seed=3, sigma=0.1)  # draw 1: the warm-up allocates everything
    chain.generation(G, 3, 0.1)
    same(arc, chain.ref, "before the capture")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = evolution.generation(d_init, G, seed=3, sigma=0.1)
    seen = []
    for replay in range(3):
        graph.replay()
        torch.cuda.synchronize()
        _check_generation(res, chain.generation(G, 3, 0.1), S)  # draws 2, 3, 4: the counter lives on the device
        same(arc, chain.ref, f"replay {replay}")
        seen.append(_np(res.genomes).copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    arc.check_errors()
    arc.close(), gen.close(), ev.close()


def test_a_refused_pair():
    G, S = 6, 3
    ev, names, score, arc, gen, init, mean = _setup("loderunner", S)
    rng = np.random.default_rng(2)
    genomes = mean + _genomes(rng, G, arc.n_params)
    bad = genomes.copy()
    bad[2, -1] = np.inf  # the last bias: every logit of that tile is inf

    def run(rows, archive_):
        out = gen.generate(_t(rows), _t(init))
        objective, behaviours = score(out.levels.view(len(rows) * S, *ev.map_shape))
        agg = evo.aggregate(objective.reshape(len(rows), S), behaviours.reshape(len(rows), S, -1), out.n_step)
        return out, agg, archive_.add(_t(rows), agg.objective, agg.behaviours)

    out, agg, added = run(bad, arc)
    assert (_np(out.n_step)[2] == -1).all() and (np.delete(_np(out.n_step), 2, 0) >= 0).all()
    assert _np(agg.valid).tolist() == [1, 1, 0, 1, 1, 1]
    assert np.isnan(_np(agg.objective)[2]) and np.isnan(_np(agg.behaviours)[2]).all()
    assert _np(added.status)[2] == 3 and _np(added.cell)[2] == -1 and _np(added.counts)[2] == 1
    with pytest.raises(ValueError, match="non-finite"):
        gen.check_errors()
    with pytest.raises(ValueError, match="refused"):
        arc.check_errors()
    # the other genomes are placed as without it
    clean = genome_archive_for(ev, names, bins=4)
    _, agg2, added2 = run(np.delete(bad, 2, 0), clean)
    assert np.array_equal(np.delete(_np(added.status), 2), _np(added2.status))
    assert np.array_equal(np.delete(_np(added.cell), 2), _np(added2.cell))
    assert E.same_bits(np.delete(_np(agg.objective), 2), _np(agg2.objective))
    a, b = arc.elites(), clean.elites()
    assert np.array_equal(_np(a.cells), _np(b.cells)) and E.same_bits(_np(a.genomes), _np(b.genomes))
    clean.check_errors()
    arc.close(), clean.close(), gen.close(), ev.close()
