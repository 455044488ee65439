"""Level measures, pairwise Hamming diversity and the behaviour vector of Lode Runner maps
(include/pcgrl_amd_loderunner_measures.h) on the GPU: every fixture recorded from the reference
(tests/golden/loderunner_measures/, tools/gen_golden_loderunner_measures.py) through LodeRunnerEvaluator, caller maps at every
byte offset with guarded outputs, batch sizes around a wave, every optional output left out, masked tile ids next to the
evaluator's own error bit, behaviour() on the committed stock levels of tests/golden/loderunner/, graph capture, two evaluators
on two streams and a group whose sum exceeds 32 bits.

Equality: every integer exact; every float form but entropy bit-equal to the reference's recorded answer; entropy bit-equal to
measures_numpy in this process (the same host log built both tables) -- the convention of tests/test_gpu_smb_measures.py."""
import glob
import os

import numpy as np
import pytest

import measures_numpy as mn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from conftest import GOLDEN  # noqa: E402

DEV = "cuda:0"
T = 8
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "loderunner_measures", "*.npz")))
STOCK = sorted(glob.glob(os.path.join(GOLDEN, "loderunner", "stock_*.npz")))
REF_KEYS = (("emptiness", "ref_emptiness"), ("symmetry-horizontal", "ref_sym_hor"), ("symmetry-vertical", "ref_sym_ver"),
            ("symmetry", "ref_sym"), ("co-occurance", "ref_co"))
STAT_KEYS = ["player", "enemies", "gold", "win", "path-length"]


def fixture_id(path):
    return os.path.basename(path)[:-4]


def fixture_shape(path):
    H, W = (int(v) for v in fixture_id(path).split("_")[1].split("x"))
    return H, W


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _evaluator(shape):
    from control_pcgrl_amd import LodeRunnerEvaluator
    return LodeRunnerEvaluator(shape, DEV)


def _check_measures(m, grids, what):
    """a measures() result against the numpy rules on `grids` (uint8 [n, H, W] on the host)"""
    n, H, W = grids.shape
    cnt, mat = mn.counts(grids, T), mn.matches(grids, T)
    assert m.counts.dtype == torch.int32 and m.match.dtype == torch.int32 and tuple(m.counts.shape) == (n, T)
    assert np.array_equal(_np(m.counts), cnt), what
    assert np.array_equal(_np(m.match), mat), what
    bc = mn.bc_from_integers(cnt, mat, H, W, T)
    assert set(m.bc) == set(mn.BC_NAMES)
    for key in mn.BC_NAMES:
        assert m.bc[key].dtype == torch.float64
        assert np.array_equal(_bits(_np(m.bc[key])), _bits(bc[key])), (what, key)
    assert np.array_equal(_bits(_np(m.tile_fractions)), _bits(mn.tile_fractions(cnt, H * W))), what
    assert m.entropy is m.bc["entropy"] and m.emptiness is m.bc["emptiness"] and tuple(m.forms.shape) == (n, 5 + T)


def _check_diversity(d, grids, K, what, want=None):
    """a diversity() result against the numpy rules (or the recorded integers `want` = (S, nearest, nearest_idx))"""
    n, H, W = grids.shape
    if want is None:
        S, near, idx, mats = mn.diversity(grids, T, K)
    else:
        (S, near, idx), mats = want, None
    assert d.hamming_sum.dtype == torch.int64 and d.nearest.dtype == torch.int32 and d.nearest_idx.dtype == torch.int32
    assert np.array_equal(_np(d.hamming_sum), S), what
    assert np.array_equal(_np(d.nearest), near), what
    assert np.array_equal(_np(d.nearest_idx), idx), what
    assert np.array_equal(_bits(_np(d.div_score)), _bits(mn.div_score(S, K, H * W))), what
    assert np.array_equal(_bits(_np(d.diversity_bonus)), _bits(mn.diversity_bonus(S, K, H * W))), what
    if d.pairwise is not None and mats is not None:
        assert np.array_equal(_np(d.pairwise), mats), what


def _same_measures(a, b):
    assert torch.equal(a.counts, b.counts) and torch.equal(a.match, b.match) and torch.equal(a.forms, b.forms)
    assert (a.entropy is None and b.entropy is None) or torch.equal(a.entropy, b.entropy)


def _same_diversity(a, b):
    assert torch.equal(a.hamming_sum, b.hamming_sum) and torch.equal(a.scores, b.scores)
    assert torch.equal(a.nearest, b.nearest) and torch.equal(a.nearest_idx, b.nearest_idx)
    assert (a.pairwise is None and b.pairwise is None) or torch.equal(a.pairwise, b.pairwise)


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_fixtures_through_evaluator_measures(path):
    z = np.load(path)
    H, W = fixture_shape(path)
    ev = _evaluator((H, W))
    grids = z["grids"]
    m = ev.measures(torch.as_tensor(grids))
    assert np.array_equal(_np(m.counts), z["counts"]) and np.array_equal(_np(m.match), z["match"])
    _check_measures(m, grids, fixture_id(path))  # (entropy: bit-equal to measures_numpy on this host)
    for key, name in REF_KEYS:  # the reference's own answers, bit for bit
        assert np.array_equal(_bits(_np(m.bc[key])), _bits(z[name])), key
    assert np.array_equal(_bits(_np(m.tile_fractions)), _bits(z["ref_tile_fractions"]))
    err = np.abs(_np(m.entropy) - z["ref_entropy"]).max()
    print(f"{fixture_id(path)}: entropy differs from the recorded one by at most {err:.3e}")
    assert err <= 1e-13
    # without entropy: the same integers, no table
    m2 = ev.measures(torch.as_tensor(grids), entropy=False)
    assert m2.entropy is None and "entropy" not in m2.bc
    assert torch.equal(m2.counts, m.counts) and torch.equal(m2.match, m.match) and torch.equal(m2.forms, m.forms)
    # a single map (3-D and 2-D) and no maps
    for one in (ev.measures(torch.as_tensor(grids[-1:])), ev.measures(grids[-1])):
        assert torch.equal(one.counts, m.counts[-1:]) and torch.equal(one.match, m.match[-1:])
        assert torch.equal(one.entropy, m.entropy[-1:])
    none = ev.measures(torch.empty((0, H, W), dtype=torch.uint8))
    assert tuple(none.counts.shape) == (0, T) and tuple(none.bc["symmetry"].shape) == (0,)
    with pytest.raises(ValueError, match="shape"):
        ev.measures(torch.zeros((2, H, W + 1), dtype=torch.uint8))
    ev.check_errors()
    ev.close()
    assert ev._entropy_tab is None  # close() drops the table
    with pytest.raises(RuntimeError, match="closed"):
        ev.measures(torch.as_tensor(grids))


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_fixtures_through_evaluator_diversity(path):
    z = np.load(path)
    H, W = fixture_shape(path)
    ev = _evaluator((H, W))
    gi, seen = 0, set()
    for c in range(len(z["div_K"])):
        K, G = int(z["div_K"][c]), int(z["div_G"][c])
        lo, hi = int(z["div_off"][c]), int(z["div_off"][c + 1])
        sel = z["grids"][z["div_idx"][lo:hi]]
        what = f"{fixture_id(path)} K={K} G={G}"
        d = ev.diversity(torch.as_tensor(sel), group=K, pairwise=True)
        want = (z["div_sum"][gi:gi + G], z["div_nearest"][lo:hi], z["div_nearest_idx"][lo:hi])
        _check_diversity(d, sel, K, what, want=want)
        # the reference's own answers, bit for bit
        assert np.array_equal(_bits(_np(d.div_score)), _bits(z["div_ref_score"][gi:gi + G])), what
        assert np.array_equal(_bits(_np(d.diversity_bonus)), _bits(z["div_ref_bonus"][gi:gi + G])), what
        # the matrix: symmetric, zero diagonal, and it is what the sums and the nearest maps come from
        pw = d.pairwise
        assert tuple(pw.shape) == (G, K, K) and pw.dtype == torch.int32
        assert torch.equal(pw, pw.transpose(1, 2)) and int(pw.diagonal(dim1=1, dim2=2).abs().sum()) == 0
        assert torch.equal(pw.sum((1, 2), dtype=torch.int64), d.hamming_sum)
        if K <= 5 or H * W <= 260:  # (the host's own matrix: small cases only, the identities above hold for all)
            assert np.array_equal(_np(pw), mn.diversity(sel, T, K)[3]), what
        off = pw + torch.eye(K, dtype=torch.int32, device=pw.device)[None] * (H * W + 1)
        assert torch.equal(off.min(2).values.reshape(-1), d.nearest), what
        assert torch.equal(torch.gather(pw, 2, d.nearest_idx.view(G, K, 1).long()).reshape(-1), d.nearest), what
        if G == 1:  # group=None is one group of everything
            whole = ev.diversity(torch.as_tensor(sel))
            assert whole.pairwise is None
            _same_diversity(whole, ev.diversity(torch.as_tensor(sel), group=K))
            assert torch.equal(whole.hamming_sum, d.hamming_sum) and torch.equal(whole.nearest_idx, d.nearest_idx)
        seen.add((K, G))
        gi += G
    assert seen == {(K, G) for K in (2, 3, 5, 64, 65, 130) for G in (1, 3)}
    for group in (1, 0, 7):
        with pytest.raises(ValueError, match="group"):
            ev.diversity(torch.as_tensor(z["grids"][:12]), group=group)
    ev.check_errors()
    ev.close()


GUARD = 64


class Guarded:
    """a device buffer of `nbytes` with GUARD bytes of 0xA5 on either side; .ptr is the payload's address (64-byte aligned)"""

    def __init__(self, nbytes, dtype, shape):
        self.nbytes = nbytes
        self.raw = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.ptr = self.raw.data_ptr() + GUARD
        self.dtype, self.shape = dtype, shape

    def value(self):
        return self.raw[GUARD:GUARD + self.nbytes].view(self.dtype).reshape(self.shape)

    def intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all()) and bool((self.raw[GUARD + self.nbytes:] == 0xA5).all())


def _outputs(L, H, W, n, K):
    return {"counts": Guarded(n * T * 4, torch.int32, (n, T)), "match": Guarded(n * 3 * 4, torch.int32, (n, 3)),
            "forms": Guarded(n * 13 * 8, torch.float64, (n, 13)), "entropy": Guarded(n * 8, torch.float64, (n,)),
            "scratch": Guarded(int(L.pcgrl_loderunner_diversity_scratch_bytes(H, W, n)), torch.int64, (-1,)),
            "sum": Guarded(n // K * 8, torch.int64, (n // K,)), "scores": Guarded(n // K * 16, torch.float64, (n // K, 2)),
            "nearest": Guarded(n * 4, torch.int32, (n,)), "nearest_idx": Guarded(n * 4, torch.int32, (n,)),
            "pairwise": Guarded(n * K * 4, torch.int32, (n // K, K, K))}


@pytest.mark.parametrize("shape", [(5, 7), (8, 12)], ids=["5x7", "8x12"])
def test_caller_maps_at_every_byte_offset_with_guarded_outputs(shape):
    """a batch of 3 maps placed 0 .. 15 bytes into a larger buffer (at 5 x 7 a map is 35 bytes, so the maps of one batch start
    at three different offsets mod 16).  The C entry points write into guarded buffers: nothing outside an output is
    touched, and every result equals the aligned one."""
    from control_pcgrl_amd import _lib
    L = _lib.lib()
    (H, W), n, K = shape, 3, 3
    rng = np.random.default_rng(35)
    grids = rng.integers(0, T, size=(n, H, W), dtype=np.uint8)
    ev = _evaluator((H, W))
    tab = ev._entropy_table()
    stream = torch.cuda.current_stream().cuda_stream
    first = None
    for start in range(16):
        big = torch.full((start + n * H * W + 64,), 6, dtype=torch.uint8, device=DEV)
        view = big[start:start + n * H * W].view(n, H, W)
        view.copy_(torch.as_tensor(grids))
        assert view.data_ptr() % 16 == start
        m = ev.measures(view)
        d = ev.diversity(view, pairwise=True)
        out = _outputs(L, H, W, n, K)
        assert out["scratch"].nbytes == n * (3 * ((H * W + 63) // 64) + 1) * 8
        assert L.pcgrl_loderunner_measures_for_grids(H, W, n, view.data_ptr(), out["counts"].ptr, out["match"].ptr,
                                                     out["forms"].ptr, out["entropy"].ptr, tab.data_ptr(), stream) == 0
        assert L.pcgrl_loderunner_diversity_for_grids(H, W, n, view.data_ptr(), K, out["scratch"].ptr, out["sum"].ptr,
                                                      out["scores"].ptr, out["nearest"].ptr, out["nearest_idx"].ptr,
                                                      out["pairwise"].ptr, stream) == 0
        torch.cuda.synchronize()
        assert all(g.intact() for g in out.values()), [k for k, g in out.items() if not g.intact()]
        assert torch.equal(out["counts"].value(), m.counts) and torch.equal(out["match"].value(), m.match)
        assert torch.equal(out["forms"].value(), m.forms) and torch.equal(out["entropy"].value(), m.entropy)
        assert torch.equal(out["sum"].value(), d.hamming_sum) and torch.equal(out["scores"].value(), d.scores)
        assert torch.equal(out["nearest"].value(), d.nearest) and torch.equal(out["nearest_idx"].value(), d.nearest_idx)
        assert torch.equal(out["pairwise"].value(), d.pairwise)
        assert bool((big[:start] == 6).all()) and bool((big[start + n * H * W:] == 6).all())  # (the input is only read)
        if first is None:
            _check_measures(m, grids, "aligned")
            _check_diversity(d, grids, K, "aligned")
            first = (m, d)
        else:  # equal to the aligned call
            _same_measures(m, first[0])
            _same_diversity(d, first[1])
    ev.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_a_wave(n):
    H, W = 8, 12
    rng = np.random.default_rng(100 + n)
    grids = rng.integers(0, T, size=(n, H, W), dtype=np.uint8)
    ev = _evaluator((H, W))
    _check_measures(ev.measures(torch.as_tensor(grids)), grids, f"n={n}")
    if n >= 2:
        _check_diversity(ev.diversity(torch.as_tensor(grids), pairwise=True), grids, n, f"n={n}")
    else:
        with pytest.raises(ValueError, match="group"):
            ev.diversity(torch.as_tensor(grids))
    ev.check_errors()
    ev.close()


def test_each_optional_output_left_out():
    """entropy=False, then the C entry points with each optional output NULL in turn: what is written equals the full call,
    what is not asked for is never touched"""
    from control_pcgrl_amd import _lib
    L = _lib.lib()
    H, W, n, K = 5, 7, 10, 5
    rng = np.random.default_rng(57)
    grids = rng.integers(0, T, size=(n, H, W), dtype=np.uint8)
    g = torch.as_tensor(grids).to(DEV)
    ev = _evaluator((H, W))
    m, d = ev.measures(g), ev.diversity(g, group=K, pairwise=True)
    _check_measures(m, grids, "full")
    _check_diversity(d, grids, K, "full")
    m0 = ev.measures(g, entropy=False)
    assert m0.entropy is None and set(m0.bc) == set(mn.BC_NAMES) - {"entropy"} and torch.equal(m0.forms, m.forms)
    d0 = ev.diversity(g, group=K)
    assert d0.pairwise is None and torch.equal(d0.hamming_sum, d.hamming_sum) and torch.equal(d0.nearest_idx, d.nearest_idx)
    tab = ev._entropy_table()
    stream = torch.cuda.current_stream().cuda_stream
    for skip in (("forms",), ("entropy",), ("forms", "entropy")):
        out = _outputs(L, H, W, n, K)
        ptr = {k: (None if k in skip else out[k].ptr) for k in out}
        assert L.pcgrl_loderunner_measures_for_grids(H, W, n, g.data_ptr(), ptr["counts"], ptr["match"], ptr["forms"],
                                                     ptr["entropy"], None if "entropy" in skip else tab.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert all(v.intact() for v in out.values())
        assert torch.equal(out["counts"].value(), m.counts) and torch.equal(out["match"].value(), m.match)
        for k, want in (("forms", m.forms), ("entropy", m.entropy)):
            if k in skip:
                assert bool((out[k].raw == 0xA5).all()), k
            else:
                assert torch.equal(out[k].value(), want), k
    optional = ("scores", "nearest", "nearest_idx", "pairwise")
    want = {"scores": d.scores, "nearest": d.nearest, "nearest_idx": d.nearest_idx, "pairwise": d.pairwise}
    for skip in [(k,) for k in optional] + [("scores", "nearest", "nearest_idx"), optional]:
        out = _outputs(L, H, W, n, K)
        ptr = {k: (None if k in skip else out[k].ptr) for k in out}
        assert L.pcgrl_loderunner_diversity_for_grids(H, W, n, g.data_ptr(), K, ptr["scratch"], ptr["sum"], ptr["scores"],
                                                      ptr["nearest"], ptr["nearest_idx"], ptr["pairwise"], stream) == 0
        torch.cuda.synchronize()
        assert all(v.intact() for v in out.values())
        assert torch.equal(out["sum"].value(), d.hamming_sum), skip
        for k in optional:
            if k in skip:
                assert bool((out[k].raw == 0xA5).all()), (skip, k)
            else:
                assert torch.equal(out[k].value(), want[k]), (skip, k)
    ev.close()


def test_tile_ids_are_masked_to_three_bits():
    """ids >= 8 alias onto the eight counted tiles and no error bit is set by measures() / diversity(); the evaluator's own
    convention (above 7 reads as empty, error bit 0) is untouched and differs"""
    rng = np.random.default_rng(7)
    H, W = 5, 7
    raw = rng.integers(0, 256, size=(10, H, W), dtype=np.uint8)
    raw[0], raw[1], raw[2], raw[3] = 7, 8, 255, 0  # all-7, all-8 (= all-0), all-255 (= all-7), all-0
    kept = mn.mask_ids(raw, T)
    assert kept.max() == 7 and raw.max() > 7
    ev = _evaluator((H, W))
    a, b = ev.measures(torch.as_tensor(raw)), ev.measures(torch.as_tensor(kept))
    _same_measures(a, b)
    _check_measures(a, raw, "masked")
    assert a.counts[0].tolist() == [0] * 7 + [35] == a.counts[2].tolist()  # with T = 8 id 7 is a counted tile
    assert a.counts[1].tolist() == [35] + [0] * 7 == a.counts[3].tolist()
    assert a.match[0].tolist() == [2 * 7, 5 * 3, 4 * 35]
    assert int(a.counts.sum(1).min()) == 35 == int(a.counts.sum(1).max())  # every masked id is counted
    d = ev.diversity(torch.as_tensor(raw), group=5, pairwise=True)
    _check_diversity(d, raw, 5, "masked")
    pw = d.pairwise[0]
    assert int(pw[0, 2]) == 0 and int(pw[1, 3]) == 0 and int(pw[0, 1]) == 35  # 7 = 255, 8 = 0, 7 against 0: once a cell
    _same_diversity(d, ev.diversity(torch.as_tensor(kept), group=5, pairwise=True))
    ev.check_errors()  # silent: the measures set no error
    # the evaluator's own launch on the same bytes does
    ev.evaluate(torch.as_tensor(raw), gold_cap=0)
    with pytest.raises(ValueError, match="above 7"):
        ev.check_errors()
    ev.measures(torch.as_tensor(raw))
    ev.check_errors()
    ev.close()


def _stock():
    grids = np.concatenate([np.load(f)["grids"] for f in STOCK])
    stats = np.concatenate([np.load(f)["stats"] for f in STOCK])
    assert grids.shape[1:] == (8, 12) and len(STOCK) == 4 and list(np.load(STOCK[0])["stat_keys"]) == STAT_KEYS
    return grids, stats


def test_behaviour_on_the_stock_levels(monkeypatch):
    """get_bc per name, in order: a statistic is the recorded one, a measure the numpy rule's, bit for bit"""
    from control_pcgrl_amd import LODERUNNER_BC_NAMES
    grids, stats = _stock()
    n = len(grids)
    cnt, mat = mn.counts(grids, T), mn.matches(grids, T)
    want = dict(mn.bc_from_integers(cnt, mat, 8, 12, T))
    want.update({k: stats[:, i] for i, k in enumerate(STAT_KEYS)})
    want["NONE"] = np.zeros(n)
    ev = _evaluator((8, 12))
    g = torch.as_tensor(grids).to(DEV)
    calls = []
    evaluate, measures = ev.evaluate, ev.measures
    monkeypatch.setattr(ev, "evaluate", lambda *a, **k: (calls.append(("evaluate", k)), evaluate(*a, **k))[1])
    monkeypatch.setattr(ev, "measures", lambda *a, **k: (calls.append(("measures", k)), measures(*a, **k))[1])

    def check(names, launches):
        del calls[:]
        b = ev.behaviour(g, names)
        assert b.dtype == torch.float64 and tuple(b.shape) == (n, len(names)) and b.device.type == "cuda"
        for j, k in enumerate(names):
            assert np.array_equal(_bits(_np(b[:, j])), _bits(want[k])), (names, k)
        assert calls == launches, (names, calls)
        return b

    ev_call, no_ent, with_ent = ("evaluate", {"gold_cap": 0}), ("measures", {"entropy": False}), ("measures", {"entropy": True})
    # the quality-diversity loop's pairs (configs/evo/batch.yaml)
    check(("emptiness", "path-length"), [ev_call, no_ent])
    check(("symmetry", "path-length"), [ev_call, no_ent])
    # all names at once, and in another order with a repeat
    check(tuple(LODERUNNER_BC_NAMES), [ev_call, with_ent])
    check(("NONE", "co-occurance", "win", "entropy", "win", "symmetry-vertical"), [ev_call, with_ent])
    # only statistics: no measures launch and no measures output; only measures: no evaluation; "NONE" alone: neither
    ev._entropy_tab = None
    check(("path-length", "win", "gold"), [ev_call])
    check(("player", "NONE"), [ev_call])
    check(("symmetry", "emptiness"), [no_ent])
    assert ev._entropy_tab is None  # (entropy was never named: not even its table)
    check(("entropy",), [with_ent])
    assert float(check(("NONE",), []).abs().sum()) == 0.0
    assert tuple(ev.behaviour(g, "symmetry").shape) == (n, 1)  # a single name
    # a list as well as a tuple; an unknown name raises and lists the known ones, before any launch
    check(["symmetry-horizontal"], [no_ent])
    del calls[:]
    for bad in (("emptiness", "brightness"), ("sol-length",), ("none",)):
        with pytest.raises(ValueError, match="known names.*path-length.*co-occurance.*NONE"):
            ev.behaviour(g, bad)
    assert calls == []
    ev.check_errors()
    ev.close()


def test_measures_and_diversity_captured_in_one_graph():
    """measures() + diversity() + behaviour() captured on a side stream after one eager call of the same size (which uploads
    the entropy table and sizes the evaluator's workspace), replayed on new maps written into the captured input"""
    n, K, shape = 64, 32, (8, 12)
    rng = np.random.default_rng(72)
    ev = _evaluator(shape)
    g = torch.as_tensor(rng.integers(0, T, size=(n,) + shape, dtype=np.uint8)).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ev.measures(g)
        ev.diversity(g, group=K, pairwise=True)
        ev.behaviour(g, ("symmetry", "path-length"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            m = ev.measures(g)
            d = ev.diversity(g, group=K, pairwise=True)
            b = ev.behaviour(g, ("symmetry", "path-length"))
    torch.cuda.current_stream().wait_stream(side)
    for t in range(3):
        host = rng.integers(0, T, size=(n,) + shape, dtype=np.uint8)
        g.copy_(torch.as_tensor(host))
        graph.replay()
        torch.cuda.synchronize()
        _check_measures(m, host, f"replay {t}")
        _check_diversity(d, host, K, f"replay {t}")
        _same_measures(m, ev.measures(g))
        _same_diversity(d, ev.diversity(g, group=K, pairwise=True))
        assert torch.equal(b, ev.behaviour(g, ("symmetry", "path-length")))
        assert torch.equal(b[:, 0], m.bc["symmetry"])
    ev.check_errors()
    ev.close()


def test_two_evaluators_on_two_streams():
    shapes, n, K = ((8, 12), (15, 31)), 130, 65
    rng = np.random.default_rng(2)
    hosts = [rng.integers(0, T, size=(n,) + s, dtype=np.uint8) for s in shapes]
    evs = [_evaluator(s) for s in shapes]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    gs = [torch.as_tensor(h).to(DEV) for h in hosts]
    torch.cuda.synchronize()
    results = [[], []]
    for _ in range(4):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                results[i].append((evs[i].measures(gs[i]), evs[i].diversity(gs[i], group=K, pairwise=True)))
    torch.cuda.synchronize()
    for i in (0, 1):
        for m, d in results[i]:
            _check_measures(m, hosts[i], f"evaluator {i}")
            _check_diversity(d, hosts[i], K, f"evaluator {i}")
        evs[i].check_errors()
        evs[i].close()


def test_sum_beyond_32_bits():
    """With 8 tiles a cell of K maps has at most K^2 - 8 (K / 8)^2 = 7 K^2 / 8 ordered pairs that differ (the eight tiles
    equally often), so at the largest map of 512 cells S <= 448 K^2: S >= 2^32 needs K >= 3 097.  K = 3 104 maps of 16 x 32,
    map i all of tile i % 8, in one group: S = 512 * (3104^2 - 8 * 388^2) = 4 316 397 568 > 2^32; 9.6 million pairs of 24 words,
    well under a second."""
    n, H, W = 3104, 16, 32
    tiles = torch.arange(n, device=DEV) % 8
    grids = tiles.to(torch.uint8)[:, None, None].expand(n, H, W).contiguous()
    ev = _evaluator((H, W))
    d = ev.diversity(grids)
    S = 512 * (3104 * 3104 - 8 * 388 * 388)
    assert S == 4316397568 > 1 << 32 and mn.hamming_sum(_np(grids), T) == S
    assert int(d.hamming_sum[0]) == S
    assert np.array_equal(_bits(_np(d.div_score)), _bits(mn.div_score([S], n, H * W)))
    assert np.array_equal(_bits(_np(d.diversity_bonus)), _bits(mn.diversity_bonus([S], n, H * W)))
    assert int(d.nearest.abs().sum()) == 0  # every map has a copy
    want = np.arange(n, dtype=np.int32) % 8  # ... the lowest one: i % 8, and for the first eight maps their second copy
    want[:8] += 8
    assert np.array_equal(_np(d.nearest_idx), want)
    m = ev.measures(grids[6:10])
    assert m.counts.tolist() == [[512 if t == k else 0 for t in range(8)] for k in (6, 7, 0, 1)]
    assert m.match.tolist() == [[8 * 32, 16 * 16, 4 * 512]] * 4
    ev.check_errors()
    ev.close()
