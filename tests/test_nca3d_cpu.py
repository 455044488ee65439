"""The numpy twins of the 3-D NCA level generator (control_pcgrl_amd/nca3d.py; include/pcgrl_amd_nca3d.h)
against the float64 statement of the step (tests/nca3d_reference.py), against the roll-outs recorded from the reference's NCA3D
class (tools/gen_golden_nca3d.py -> tests/golden/nca3d), the bordered map, the order of layer 1, the error rules and the
refusals.  No GPU."""
import glob
import os

import numpy as np
import pytest

import nca3d_reference as r3
from conftest import GOLDEN
from control_pcgrl_amd import Nca3dGenerator, all_holes, fixed_holes, generator3d_for, nca, nca3d

FILES = sorted(glob.glob(os.path.join(GOLDEN, "nca3d", "*.npz")))
EXEMPT_CAP = 0.02      # of the recorded cells of a file
MAX_FILE_BYTES = 100 * 1024


def load(path):
    return dict(np.load(path))


def holes_of(z, i):
    return z["hole_pairs"][z["hole"][i]] if bool(z["holey"]) else None


# ---- the float64 statement ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,shape,holey", [(2, (3, 3, 3), False), (2, (5, 4, 3), True), (3, (3, 4, 5), True), (5, (7, 7, 7), True),
                                           (5, (3, 4, 5), False), (8, (6, 5, 4), False), (8, (4, 7, 5), True)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_twin_equals_the_float64_reference(T, shape, holey):
    """random genomes, five steps of three seeds along the twin's own trajectory: on every cell that the recorder's rule does
    not exempt, the twin's pick is the float64 argmax.  (The float32 logits stay within 1e-5 of the float64 ones, a hundredth
    of the exemption's margin.)"""
    rng = np.random.default_rng(4400 + T + sum(shape))
    pairs = all_holes(shape)
    cells = exempted = wrong = 0
    err = 0.0
    for w in r3.genomes(rng, 2, T):
        cur = r3.seeds(rng, (3,), shape, T)
        holes = pairs[rng.integers(0, len(pairs), 3)] if holey else None
        for _ in range(5):
            nxt, l32 = nca3d.stepped(w, cur, holes, n_tiles=T)
            for s in range(3):
                l64 = r3.logits64(w, cur[s], T, None if holes is None else holes[s])
                ex = r3.exempt(l64)
                cells += ex.size
                exempted += int(ex.sum())
                wrong += int((nxt[s] != np.argmax(l64, axis=0))[~ex].sum())
                err = max(err, float(np.abs(l64 - l32[s]).max()))
            cur = nxt
    print(f"T = {T} {shape}: exempt share {exempted / cells:.5f} of {cells} cells, {wrong} disagree, max |float64 - float32| {err:.2e}")
    assert wrong == 0 and exempted / cells <= EXEMPT_CAP and err < 1e-5


# ---- the fixtures --------------------------------------------------------------------------------------------------------------

def test_fixture_set():
    names = [os.path.basename(p) for p in FILES]
    assert names == ["nca3d_T2_3x3x3_plain.npz", "nca3d_T2_5x4x3_holey.npz", "nca3d_T5_3x4x5_plain_m0.npz",
                     "nca3d_T5_3x4x5_plain_m2.npz", "nca3d_T5_3x4x5_plain_m5.npz", "nca3d_T5_7x7x7_holey_m0.npz",
                     "nca3d_T5_7x7x7_holey_m2.npz", "nca3d_T5_7x7x7_holey_m5.npz"], names
    mutations = {2: set(), 5: set()}
    for path in FILES:
        z = load(path)
        T = int(z["n_tiles"])
        assert z["weights"].shape[1] == nca3d.n_params(T) and int(z["n_steps"]) == 10
        mutations[T] |= set(z["n_mutations"].tolist())
        clean = z["clean"]
        assert clean.sum() >= 8
        assert (z["n_step"][clean] < 9).any() and (z["n_step"][clean] == 9).any()
        if bool(z["holey"]):
            shape = z["init"].shape[1:]
            pairs = z["hole_pairs"]
            assert np.array_equal(pairs[0], fixed_holes(shape))
            listed = {p.tobytes() for p in all_holes(shape)}
            assert all(p.tobytes() in listed for p in pairs[1:])
            Z, Y, X = shape
            ent = pairs[1:, 0]
            assert (ent[:, 2] == 0).any() and (ent[:, 2] == X + 1).any() and (ent[:, 1] == 0).any() and (ent[:, 1] == Y + 1).any()
            assert set(z["hole"].tolist()) == set(range(len(pairs)))  # every pair has trajectories
        else:
            assert z["hole_pairs"].shape == (0, 2, 3)
    assert mutations == {2: {0, 2, 5}, 5: {0, 2, 5}}
    assert any((~load(p)["clean"]).any() for p in FILES)  # exempt cells are exercised too


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_exempt_cap_and_size(path):
    z = load(path)
    share = z["exempt"].mean()
    print(f"exempt share {share:.5f}, {os.path.getsize(path)} bytes")
    assert share <= EXEMPT_CAP
    assert os.path.getsize(path) <= MAX_FILE_BYTES


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_twin_reproduces_every_recorded_step(path):
    z = load(path)
    T = int(z["n_tiles"])
    cells = wrong = 0
    for i in range(len(z["init"])):
        w = nca3d.unpack_weights(z["weights"][z["genome"][i]], T)
        prev = z["init"][i]
        for step in range(int(z["n_step"][i]) + 1):
            nxt, _ = nca3d.stepped(w, prev, holes_of(z, i))
            keep = ~z["exempt"][i, step]
            cells += int(keep.sum())
            wrong += int((nxt != z["frames"][i, step])[keep].sum())
            prev = z["frames"][i, step]  # the reference's own trajectory
    print(f"{cells} non-exempt cells, {wrong} disagree")
    assert cells > 0 and wrong == 0


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_twin_reproduces_clean_trajectories(path):
    z = load(path)
    T, n_steps = int(z["n_tiles"]), int(z["n_steps"])
    for i in np.flatnonzero(z["clean"]):
        out = nca3d.generated(z["weights"][z["genome"][i]][None], z["init"][i][None], holes_of(z, i), n_steps, n_tiles=T)
        assert out.error_bits == 0
        assert out.n_step[0, 0] == z["n_step"][i]
        assert np.array_equal(out.frames[0, 0], z["frames"][i])
        assert np.array_equal(out.levels[0, 0], z["frames"][i, -1])


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_unpack_weights_is_the_recorded_layout(path):
    z = load(path)
    T = int(z["n_tiles"])
    for gi in range(len(z["weights"])):
        w = nca3d.unpack_weights(z["weights"][gi], T)
        for mine, name in ((w.w1, "l1_weight"), (w.b1, "l1_bias"), (w.w2, "l2_weight"), (w.b2, "l2_bias"), (w.w3, "l3_weight"),
                           (w.b3, "l3_bias")):
            assert mine.dtype == np.float32 and mine.shape == z[name][gi].shape and np.array_equal(mine, z[name][gi]), name


# ---- the rules -----------------------------------------------------------------------------------------------------------------

def test_n_params():
    assert nca3d.n_params(2) == 2882 and nca3d.n_params(5) == 5573 and nca3d.n_params(8) == 8264
    assert all(nca3d.n_params(T) == 897 * T + 1088 for T in range(2, 9))
    assert all(nca3d.n_params(T) != nca.n_params(U) for T in range(2, 9) for U in range(2, 9))
    assert nca3d.sigmoid32 is nca.sigmoid32


def test_bordered_against_all_holes():
    """the first and the last pair of all_holes: the border, foot and head of both holes, the interior untouched"""
    rng = np.random.default_rng(1)
    for shape in ((7, 7, 7), (3, 4, 5)):
        g = r3.seeds(rng, (), shape, 5)
        pairs = all_holes(shape)
        for pair in (pairs[0], pairs[-1]):
            b = nca3d.bordered(g, pair, border_tile=1, empty_tile=0)
            assert b.dtype == np.uint8 and b.shape == tuple(s + 2 for s in shape)
            assert np.array_equal(b[1:-1, 1:-1, 1:-1], g)
            ring = np.ones(b.shape, bool)
            ring[1:-1, 1:-1, 1:-1] = False
            want_air = {(int(z) + dz, int(y), int(x)) for z, y, x in pair for dz in (0, 1)}
            assert {tuple(int(v) for v in c) for c in np.argwhere(ring & (b == 0))} == want_air
            assert ((b == 1) | ~ring | (b == 0)).all() and (ring & (b == 1)).sum() == ring.sum() - len(want_air)
            assert np.array_equal(b, r3.bordered64(g, pair))
        other = nca3d.bordered(g, pairs[0], border_tile=3, empty_tile=2)
        assert set(np.unique(other[ring]).tolist()) == {2, 3}
    batch = nca3d.bordered(np.zeros((2, 3, 3, 3), np.uint8), np.stack([fixed_holes((3, 3, 3))] * 2))
    assert batch.shape == (2, 5, 5, 5) and np.array_equal(batch[0], batch[1])
    with pytest.raises(ValueError, match="side face"):
        nca3d.bordered(np.zeros((3, 3, 3), np.uint8), [[0, 0, 1], [2, 4, 1]])


def test_marker_genome_moves_the_expected_cell():
    """one non-zero weight: l1.weight[o, c=1, k0=0, k1=2, k2=1] lights hidden unit o at the cell whose neighbour at
    (z - 1, y + 1, x) holds tile 1; l2 and l3 carry unit o to tile 2's logit, so exactly that cell becomes tile 2"""
    T, shape, o = 3, (3, 4, 5), 11
    P = nca3d.n_params(T)
    g = np.zeros(P, np.float32)
    g[(((o * T + 1) * 3 + 0) * 3 + 2) * 3 + 1] = 1.0           # l1.weight[o, 1, 0, 2, 1]
    g[864 * T + 32 + o * 32 + o] = 1.0                          # l2.weight[o, o]
    g[864 * T + 32 + 1056 + 2 * 32 + o] = 1.0                   # l3.weight[2, o]
    grid = np.zeros(shape, np.uint8)
    grid[0, 3, 2] = 1
    nxt, logits = nca3d.stepped(g, grid, n_tiles=T)
    want = np.zeros(shape, np.uint8)
    want[1, 2, 2] = 2  # (z + k0 - 1, y + k1 - 1, x + k2 - 1) == (0, 3, 2)
    assert np.array_equal(nxt, want)
    assert logits[2, 1, 2, 2] == 1.0 and np.count_nonzero(logits) == 1
    # in holey mode the ring is read: tile 1 is the border, so every cell with a border cell at that tap lights up too
    nxt, logits = nca3d.stepped(g, np.zeros(shape, np.uint8), fixed_holes(shape), n_tiles=T)
    seen = nca3d.bordered(np.zeros(shape, np.uint8), fixed_holes(shape))
    assert np.array_equal(nxt == 2, seen[0:3, 2:6, 1:6] == 1) and (nxt == 2).any() and (nxt == 0).any()


def test_the_order_of_layer_1_is_by_tap():
    """2^24, -2^24 and 1 at three taps of two tiles: tap order and (tile, tap) order give different float32 sums, and the twin
    takes the tap order"""
    g, m = r3.order_genome(), r3.order_map()
    w = nca3d.unpack_weights(g, 2)
    assert np.count_nonzero(w.w1) == 3 and sorted(w.w1[w.w1 != 0].tolist()) == [-2.0 ** 24, 1.0, 2.0 ** 24]
    by_tap, by_tile = r3.tap_order_layer1(g, m, 2), r3.tile_order_layer1(g, m, 2)
    assert by_tap[0, 1, 1, 1] == 1.0 and by_tile[0, 1, 1, 1] == 0.0
    nxt, logits = nca3d.stepped(g, m, n_tiles=2)
    assert np.array_equal(logits[1], np.maximum(by_tap[0], 0)) and not np.array_equal(logits[1], np.maximum(by_tile[0], 0))
    assert nxt[1, 1, 1] == 1  # logit 1 is 1 against logit 0's 0.5; under tile order it would be 0 against 0.5
    # a 3 x 3 x 3 map sees nothing beyond itself in plain mode: all 27 taps of the centre, 8 of a corner
    ones = np.zeros(nca3d.n_params(2), np.float32)
    u = nca3d.unpack_weights(ones, 2)
    u.w1[0] = 1.0
    u.w2[0, 0] = u.w3[1, 0] = 1.0
    _, logits = nca3d.stepped(ones, np.zeros((3, 3, 3), np.uint8), n_tiles=2)
    assert logits[1, 1, 1, 1] == 27.0 and logits[1, 0, 0, 0] == 8.0 and logits[1, 0, 1, 2] == 12.0


def test_generated_stops_pads_and_refuses():
    T, n_steps, shape = 2, 10, (3, 4, 5)
    zero = np.zeros((1, nca3d.n_params(T)), np.float32)
    out = nca3d.generated(zero, np.zeros((2,) + shape, np.uint8), None, n_steps)
    assert (out.n_step == 0).all() and (out.levels == 0).all() and out.frames.shape == (1, 2, n_steps) + shape
    ones = np.ones((1,) + shape, np.uint8)  # all-equal sigmoids: the first index wins, the map changes once, then stands
    for holes in (None, fixed_holes(shape)):
        out = nca3d.generated(zero, ones, holes, n_steps)
        assert out.n_step[0, 0] == 1 and (out.levels == 0).all() and (out.frames == 0).all()
        assert nca3d.generated(zero, ones, holes, 1).n_step[0, 0] == 0
    bad = ones.copy()
    bad[0, 2, 2, 2] = T
    out = nca3d.generated(zero, np.stack([ones[0], bad[0]]), None, n_steps)
    assert out.error_bits == nca3d.ERR_TILE and out.n_step.tolist() == [[1, -1]]
    assert np.array_equal(out.levels[0, 1], bad[0]) and (out.frames[0, 1] == bad[0]).all()
    inf = zero.copy()
    inf[0, -1] = np.inf  # l3.bias[T - 1]
    out = nca3d.generated(np.concatenate([zero, inf]), ones, None, n_steps)
    assert out.error_bits == nca3d.ERR_NONFINITE and out.n_step.tolist() == [[1], [-1]]
    assert np.array_equal(out.levels[1, 0], ones[0])
    # a refused hole: that seed alone, for every genome; the neighbours are what they are without it
    rng = np.random.default_rng(2)
    w, init = r3.genomes(rng, 2, T), r3.seeds(rng, (3,), shape, T)
    holes = np.stack([fixed_holes(shape)] * 3)
    good = nca3d.generated(w, init, holes, n_steps)
    holes[1, 0] = (3, 0, 2)  # z = Z: the head would be in the top ring
    out = nca3d.generated(w, init, holes, n_steps)
    assert out.error_bits == nca3d.ERR_HOLE and (out.n_step[:, 1] == -1).all() and (out.n_step[:, [0, 2]] >= 0).all()
    assert np.array_equal(out.levels[:, 1], np.stack([init[1]] * 2)) and (out.frames[:, 1] == init[1]).all()
    for name in ("levels", "n_step", "frames"):
        assert np.array_equal(getattr(out, name)[:, [0, 2]], getattr(good, name)[:, [0, 2]])
    both = init.copy()
    both[1, 0, 0, 0] = 7
    assert nca3d.generated(w, both, holes, n_steps).error_bits == nca3d.ERR_HOLE | nca3d.ERR_TILE


def test_refusals():
    with pytest.raises(ValueError, match="2-D maps"):
        Nca3dGenerator(2, (16, 16))
    with pytest.raises(ValueError, match="CPU fallback"):
        Nca3dGenerator(2, (7, 7, 7), device="cpu")
    with pytest.raises(ValueError, match="n_steps"):
        Nca3dGenerator(2, (7, 7, 7), n_steps=0, device="cpu")
    with pytest.raises(ValueError, match="border_tile"):
        Nca3dGenerator(2, (7, 7, 7), holey=True, border_tile=2, device="cpu")
    with pytest.raises(ValueError, match="2882"):
        nca3d.unpack_weights(np.zeros(2881, np.float32), 2)
    with pytest.raises(ValueError, match="no tile count"):
        nca3d.generated(np.zeros((1, 1730), np.float32), np.zeros((1, 4, 4, 4), np.uint8))
    with pytest.raises(ValueError, match="init_states"):
        nca3d.generated(np.zeros((1, 2882), np.float32), np.zeros((1, 4, 4), np.uint8))
    with pytest.raises(ValueError, match="holes must be"):
        nca3d.generated(np.zeros((1, 2882), np.float32), np.zeros((3, 4, 4, 4), np.uint8), np.zeros((2, 2, 3), np.int64))
    with pytest.raises(ValueError, match="border_tile"):
        nca3d.generated(np.zeros((1, 2882), np.float32), np.zeros((1, 4, 4, 4), np.uint8), fixed_holes((4, 4, 4)), border_tile=2)
    with pytest.raises(ValueError, match="n_tiles"):
        nca3d.stepped(np.zeros(2882, np.float32), np.zeros((3, 3, 3), np.uint8))
    with pytest.raises(TypeError, match="generator3d_for"):
        generator3d_for(object())


def test_the_unit_is_listed():
    from control_pcgrl_amd import _lib
    assert "nca3d/pcgrl_k_nca3d.hip" in _lib.UNITS and "nca3d/pcgrl_nca3d.h" in _lib.HEADERS
    assert ("pcgrl_amd_nca3d.h", _lib.NCA3D_SYMBOLS) in _lib.ABI
    assert set(_lib.NCA3D_SYMBOLS) == {"pcgrl_nca3d_create", "pcgrl_nca3d_destroy", "pcgrl_nca3d_generate",
                                       "pcgrl_nca3d_poll_error", "pcgrl_nca3d_last_error"}
    L = _lib.lib()
    assert all(hasattr(L, name) for name in _lib.NCA3D_SYMBOLS)


def test_evolution_glue_keeps_its_defaults():
    import inspect

    from control_pcgrl_amd import evo
    assert inspect.signature(evo.genome_archive_for).parameters["n_params"].default is None
    assert inspect.signature(evo.NcaEvolution.generation).parameters["holes"].default is None
    assert callable(evo.mc3d_holey_score)
