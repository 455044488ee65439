"""The numpy twins of the NCA level generator (control_pcgrl_amd/nca.py; include/pcgrl_amd_nca.h) against
the roll-outs recorded from the reference's NCA class (tools/gen_golden_nca.py -> tests/golden/nca), the stated properties of
sigmoid32, the genome layout and the refusals; for every tile count against the float64 statement of the step and the correctly
rounded sigmoid of tests/nca_reference.py, on random genomes and on the probe set the device's pick is held to.  No GPU."""
import glob
import os

import numpy as np
import pytest

import nca_reference as nr
from conftest import GOLDEN
from control_pcgrl_amd import NcaGenerator, generator_for, nca

FILES = sorted(glob.glob(os.path.join(GOLDEN, "nca", "*.npz")))
EXEMPT_CAP = 0.02  # of the recorded cells per tile count


def load(path):
    return dict(np.load(path))


def test_fixture_set():
    names = [os.path.basename(p) for p in FILES]
    assert names == ["nca_T2_16x16.npz", "nca_T3_5x7.npz", "nca_T8_16x16.npz"], names
    for path in FILES:
        z = load(path)
        T = int(z["n_tiles"])
        assert z["weights"].shape[1] == nca.n_params(T)
        if z["init"].shape[1:] == (16, 16):
            clean = z["clean"]
            assert z["weights"].shape[0] == 6 and sorted(z["n_mutations"].tolist()) == [0, 0, 5, 5, 10, 10]
            assert clean.sum() >= 16
            assert (z["n_step"][clean] < 9).any() and (z["n_step"][clean] == 9).any()
            assert (~clean).any()  # exempt cells are exercised too


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_exempt_cap(path):
    z = load(path)
    share = z["exempt"].mean()
    print(f"exempt share {share:.5f}")
    assert share <= EXEMPT_CAP


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_twin_reproduces_every_recorded_step(path):
    z = load(path)
    T = int(z["n_tiles"])
    cells = wrong = 0
    for i in range(len(z["init"])):
        w = nca.unpack_weights(z["weights"][z["genome"][i]], T)
        prev = z["init"][i]
        for step in range(int(z["n_step"][i]) + 1):
            nxt, _ = nca.stepped(w, prev)
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
    for gi in range(len(z["weights"])):
        rows = np.flatnonzero((z["genome"] == gi) & z["clean"])
        if len(rows) == 0:
            continue
        out = nca.generated(z["weights"][gi:gi + 1], z["init"][rows], n_steps, n_tiles=T)
        assert out.error_bits == 0
        assert np.array_equal(out.n_step[0], z["n_step"][rows])
        assert np.array_equal(out.frames[0], z["frames"][rows])
        assert np.array_equal(out.levels[0], z["frames"][rows, -1])


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_unpack_weights_is_the_recorded_layout(path):
    z = load(path)
    T = int(z["n_tiles"])
    for gi in range(len(z["weights"])):
        w = nca.unpack_weights(z["weights"][gi], T)
        for mine, name in ((w.w1, "l1_weight"), (w.b1, "l1_bias"), (w.w2, "l2_weight"), (w.b2, "l2_bias"), (w.w3, "l3_weight"),
                           (w.b3, "l3_bias")):
            assert mine.dtype == np.float32 and np.array_equal(mine, z[name][gi]), name


def test_n_params():
    assert nca.n_params(2) == 1730 and nca.n_params(8) == 3656
    assert all(nca.n_params(T) == 288 * T + 32 + 1056 + 33 * T for T in range(2, 9))


def test_marker_genome_moves_the_expected_cell():
    """one non-zero weight: l1.weight[o, c=1, ky=0, kx=2] lights hidden unit o at the cell whose upper-right neighbour holds tile
    1; l2 and l3 carry unit o to tile 2's logit, so exactly that cell becomes tile 2"""
    T, H, W, o = 3, 5, 7, 11
    P = nca.n_params(T)
    g = np.zeros(P, np.float32)
    g[((o * T + 1) * 3 + 0) * 3 + 2] = 1.0                      # l1.weight[o, 1, 0, 2]
    g[288 * T + 32 + o * 32 + o] = 1.0                          # l2.weight[o, o]
    g[288 * T + 32 + 1056 + 2 * 32 + o] = 1.0                   # l3.weight[2, o]
    grid = np.zeros((H, W), np.uint8)
    grid[1, 4] = 1
    nxt, logits = nca.stepped(g, grid, n_tiles=T)
    want = np.zeros((H, W), np.uint8)
    want[2, 3] = 2  # (y + ky - 1, x + kx - 1) == (1, 4)
    assert np.array_equal(nxt, want)
    assert logits[2, 2, 3] == 1.0 and np.count_nonzero(logits) == 1
    # the biases sit where the layout says
    g = np.zeros(P, np.float32)
    g[288 * T + 32 + 1056 + 32 * T + 1] = 0.5                   # l3.bias[1]
    nxt, logits = nca.stepped(g, grid, n_tiles=T)
    assert (nxt == 1).all() and (logits[1] == 0.5).all()


def test_taps_outside_the_map_are_skipped_and_order_is_by_tile_first():
    """a 1 x 1 map sees its own tile only; the summation order of layer 1 is c, ky, kx -- shown with weights whose float32
    sum depends on the order"""
    T = 2
    g = np.zeros(nca.n_params(T), np.float32)
    w = nca.unpack_weights(g, T)
    w.w1[0] = 7.0          # every tap of hidden unit 0
    w.w2[0, 0] = 1.0
    w.w3[1, 0] = 1.0
    _, logits = nca.stepped(w, np.zeros((1, 1), np.uint8))
    assert logits[1, 0, 0] == 7.0
    # 3 x 3, centre cell: taps of tile 0 first (all but the centre), then the centre's tile 1
    grid = np.zeros((3, 3), np.uint8)
    grid[1, 1] = 1
    w.w1[0] = 0.0
    w.w1[0, 1, 1, 1] = 2.0 ** 24   # tile 1 at the centre tap: added LAST
    w.w1[0, 0] = 1.0               # eight taps of tile 0: added first, 8 exactly, then 2^24 + 8 is exact
    _, logits = nca.stepped(w, grid)
    assert logits[1, 1, 1] == np.float32(2.0 ** 24 + 8)  # (tap order would give 2^24 + 4: the later ones are absorbed)


def _logit_set():
    rng = np.random.default_rng(12345)
    return np.concatenate([rng.uniform(-40, 40, 500_000), rng.normal(0, 3, 500_000)]).astype(np.float32)


def test_sigmoid32_equals_the_float64_formula():
    x = _logit_set()
    want = (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)
    got = nca.sigmoid32(x)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_sigmoid32_is_monotone_and_saturates():
    x = np.sort(np.concatenate([_logit_set()[::10], np.linspace(-120, 120, 200_001).astype(np.float32),
                                np.float32([0.0, -0.0, 17.4, -104.0, -105.0, -1e30, 1e30, np.inf, -np.inf])]))
    s = nca.sigmoid32(x)
    assert (np.diff(s) >= 0).all()
    assert nca.sigmoid32(np.float32(0.0)) == np.float32(0.5) and nca.sigmoid32(np.float32(-0.0)) == np.float32(0.5)
    assert nca.sigmoid32(np.float32(17.4)) == np.float32(1.0) and nca.sigmoid32(np.float32(1e30)) == np.float32(1.0)
    assert nca.sigmoid32(np.float32(-104.0)) == 0.0 and nca.sigmoid32(np.float32(-105.0)) == 0.0
    assert nca.sigmoid32(np.float32(-1e30)) == 0.0
    assert nca.sigmoid32(np.float32(16.0)) < np.float32(1.0) and nca.sigmoid32(np.float32(-100.0)) > 0.0
    assert np.isnan(nca.sigmoid32(np.float32(np.nan)))


def test_channels_the_kernel_skips_cannot_tie():
    """csrc/nca/pcgrl_nca.h evaluates s32 only for channels that can still win: one with lmax - l > 1, l < 12 and lmax > -87
    is skipped.  Such a pair never has equal sigmoids -- on (nearly) the smallest gap the rule admits, over the whole range."""
    l = np.concatenate([np.linspace(-89, 12, 400_001), -np.logspace(-3, 1.9, 10_000)]).astype(np.float32)
    l = l[l < 12]
    lmax = (l.astype(np.float64) + (1.0 + 2.0 ** -23)).astype(np.float32)
    for _ in range(3):  # up to the first float32 whose float32 difference exceeds 1
        short = (lmax - l) <= np.float32(1.0)
        lmax = np.where(short, np.nextafter(lmax, np.float32(np.inf)), lmax)
    skipped = ((lmax - l) > np.float32(1.0)) & (lmax > np.float32(-87.0))
    assert skipped.sum() > 300_000 and ((lmax - l)[skipped] < np.float32(1.001)).all()
    assert (nca.sigmoid32(lmax[skipped]) > nca.sigmoid32(l[skipped])).all()


@pytest.mark.parametrize("T", range(2, 9))
def test_twin_equals_the_float64_reference(T):
    """random genomes, six steps of five seeds at 9 x 13 and 16 x 16 along the twin's own trajectory: on every cell that the
    recorder's rule does not exempt, the twin's pick is the float64 argmax.  (The float32 logits stay within 1e-5 of the float64
    ones, a hundredth of the exemption's margin; measured 2.3e-6.)"""
    rng = np.random.default_rng(3800 + T)
    cells = exempted = wrong = 0
    err = 0.0
    for shape in ((9, 13), (16, 16)):
        for w in nr.genomes(rng, 2, T):
            cur = nr.seeds(rng, (5,), shape, T)
            for _ in range(6):
                nxt, l32 = nca.stepped(w, cur, n_tiles=T)
                l64 = nr.logits64(w, cur, T)
                ex = nr.exempt(l64)
                cells += ex.size
                exempted += int(ex.sum())
                wrong += int((nxt != np.argmax(l64, axis=-3))[~ex].sum())
                err = max(err, float(np.abs(l64 - l32).max()))
                cur = nxt
    print(f"T = {T}: exempt share {exempted / cells:.5f} of {cells} cells, {wrong} disagree, max |float64 - float32 logit| {err:.2e}")
    assert wrong == 0 and exempted / cells <= EXEMPT_CAP and err < 1e-5


def _probes(T):
    return nr.probe_vectors(T, np.random.default_rng(380 + T))


def test_sigmoid32_is_the_correctly_rounded_sigmoid():
    x = np.unique(np.concatenate([_probes(T).vectors.ravel() for T in range(2, 9)]).view(np.uint32)).view(np.float32)
    want, gap = nr.sigmoid_cr32(x)
    keep = gap >= nr.GAP_FLOOR
    differ = int((nca.sigmoid32(x)[keep].view(np.uint32) != want[keep].view(np.uint32)).sum())
    print(f"{len(x)} scalars, {int((~keep).sum())} excluded, {differ} differ, smallest gap {gap.min():.2e}")
    assert len(x) > 10_000 and (~keep).sum() <= 0.001 * len(x)
    assert differ == 0


@pytest.mark.parametrize("T", range(2, 9))
def test_probe_set_discriminates(T):
    """the probe set of test_gpu_nca.test_pick_on_exact_logits, from the twin alone: it holds ties and non-ties where a wrong
    pick would show, both branches of the kernel's shortcut at each threshold, and vectors on which the shortcut without its
    `lmax > -87` answers wrongly"""
    p = _probes(T)
    v, n = p.vectors, np.arange(len(p.vectors))
    assert 1000 <= len(v) <= 3000 and len(np.unique(v.view(np.uint32), axis=0)) > 0.95 * len(v)
    s = nca.sigmoid32(v)
    twin = np.argmax(s, axis=-1)
    pair = p.lo >= 0
    lo, hi = v[n, p.lo], v[n, p.hi]
    assert (lo[pair] <= hi[pair]).all() and (p.lo[pair] < p.hi[pair]).all()
    tie = s[n, p.lo] == s[n, p.hi]
    adj = p.family == "adjacent"
    band = adj & (hi > -104) & (hi < -87)
    print(f"T = {T}: {len(v)} probes; adjacent floats: {int(tie[adj].sum())} ties, {int((~tie)[adj].sum())} non-ties of "
          f"{int(adj.sum())}; in the denormal band {int(tie[band].sum())} and {int((~tie)[band].sum())}")
    assert tie[adj].sum() >= adj.sum() / 4 and (~tie)[adj].sum() >= adj.sum() / 4
    assert tie[band].any() and (~tie)[band].any()
    if T == 2:
        assert np.array_equal(twin[adj] == 0, tie[adj])  # the lower index is the answer exactly when the sigmoids tie
    for fam in ("zero", "plateau", "zeros"):
        assert tie[p.family == fam].all()
    wide = (p.family == "denormal") & (hi - lo > np.float32(1.0))
    assert tie[wide].any() and (~tie)[wide].any()
    # the shortcut's branches, in float32 as the kernel computes them
    cannot_tie = ((hi - lo) > np.float32(1.0)) & (lo < np.float32(12.0)) & (hi > np.float32(-87.0))
    for e, (below, above) in enumerate((((hi - lo) <= np.float32(1.0), (hi - lo) > np.float32(1.0)),
                                        (lo >= np.float32(12.0), lo < np.float32(12.0)),
                                        (hi <= np.float32(-87.0), hi > np.float32(-87.0)))):
        at = p.edge == e
        taken = {True: int((cannot_tie & at).sum()), False: int((~cannot_tie & at).sum())}
        print(f"  threshold {e}: {taken[True]} probes skip the rival, {taken[False]} evaluate it")
        assert taken[True] >= 3 and taken[False] >= 3 and (below & at).any() and (above & at).any()
        if e == 0:
            assert ((hi - lo) == np.float32(1.0))[at].any()
    assert ((lo == np.nextafter(np.float32(12.0), np.float32(0)))[p.edge == 1]).any() and (lo == np.float32(12.0))[p.edge == 1].any()
    assert ((hi == np.nextafter(np.float32(-87.0), np.float32(0)))[p.edge == 2]).any() and (hi == np.float32(-87.0))[p.edge == 2].any()
    # the kernel's organisation of the pick gives the twin's answer; without the guard on lmax it does not
    pick, skipped = nr.kernel_pick(v)
    assert np.array_equal(pick, twin) and skipped.any()
    assert np.array_equal(skipped[n, np.maximum(p.lo, 0)][p.edge >= 0], cannot_tie[p.edge >= 0] & (lo < hi)[p.edge >= 0])
    unguarded, _ = nr.kernel_pick(v, lmax_guard=False)
    assert (unguarded != twin).sum() >= 50
    if T > 2:
        sev = p.family == "several"
        j = np.argmax(v, axis=-1)
        assert (twin[sev] < j[sev]).sum() >= 20 and (twin[sev] == j[sev]).sum() >= 20  # ties that win, near-misses that do not
        assert (skipped[sev].sum(axis=-1) >= 1).sum() >= 20
        assert ((v[sev] == v[sev][:, :1]).all(axis=-1)).sum() >= 6  # all T equal
    # the correctly rounded sigmoid picks the same
    ref, gap = nr.pick_ref(v)
    keep = gap >= nr.GAP_FLOOR
    print(f"  {int((~keep).sum())} probes excluded")
    assert (~keep).sum() <= 0.001 * len(v) and np.array_equal(ref[keep], twin[keep])


def test_the_unit_is_listed():
    from control_pcgrl_amd import _lib
    assert "nca/pcgrl_k_nca.hip" in _lib.UNITS and "nca/pcgrl_nca.h" in _lib.HEADERS
    assert set(_lib.NCA_SYMBOLS) == {"pcgrl_nca_create", "pcgrl_nca_destroy", "pcgrl_nca_generate", "pcgrl_nca_poll_error",
                                     "pcgrl_nca_last_error"}
    L = _lib.lib()
    assert all(hasattr(L, name) for name in _lib.NCA_SYMBOLS)


def test_generated_stops_and_pads():
    T, n_steps = 2, 10
    zero = np.zeros((1, nca.n_params(T)), np.float32)
    out = nca.generated(zero, np.zeros((2, 4, 4), np.uint8), n_steps)
    assert (out.n_step == 0).all() and (out.levels == 0).all() and out.frames.shape == (1, 2, n_steps, 4, 4)
    ones = np.ones((1, 4, 4), np.uint8)  # all-equal sigmoids: the first index wins, the map changes once, then stands
    out = nca.generated(zero, ones, n_steps)
    assert out.n_step[0, 0] == 1 and (out.levels == 0).all() and (out.frames == 0).all()
    assert nca.generated(zero, ones, 1).n_step[0, 0] == 0
    bad = ones.copy()
    bad[0, 2, 2] = T
    out = nca.generated(zero, np.stack([ones[0], bad[0]]), n_steps)
    assert out.error_bits == nca.ERR_TILE and out.n_step.tolist() == [[1, -1]]
    assert np.array_equal(out.levels[0, 1], bad[0]) and (out.frames[0, 1] == bad[0]).all()
    inf = zero.copy()
    inf[0, -1] = np.inf  # l3.bias[T - 1]
    out = nca.generated(np.concatenate([zero, inf]), ones, n_steps)
    assert out.error_bits == nca.ERR_NONFINITE and out.n_step.tolist() == [[1], [-1]]
    assert np.array_equal(out.levels[1, 0], ones[0])


def test_refusals():
    with pytest.raises(NotImplementedError, match="NCA3D"):
        NcaGenerator(2, (7, 7, 7))
    with pytest.raises(NotImplementedError, match="auxiliary"):
        NcaGenerator(2, (16, 16), n_aux_chan=3)
    with pytest.raises(ValueError, match="CPU fallback"):
        NcaGenerator(2, (16, 16), device="cpu")
    with pytest.raises(ValueError, match="n_steps"):
        NcaGenerator(2, (16, 16), n_steps=0, device="cpu")
    with pytest.raises(ValueError, match="1730"):
        nca.unpack_weights(np.zeros(1729, np.float32), 2)
    with pytest.raises(ValueError, match="no tile count"):
        nca.generated(np.zeros((1, 1729), np.float32), np.zeros((1, 4, 4), np.uint8))
    with pytest.raises(TypeError, match="generator_for"):
        generator_for(object())
