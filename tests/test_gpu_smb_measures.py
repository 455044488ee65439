"""Level measures and pairwise Hamming diversity of Super Mario Bros maps (include/pcgrl_amd_smb_measures.h) on the GPU: every
fixture recorded from the reference (tests/golden/smb_measures/, tools/gen_golden_smb_measures.py) through SmbEvaluator, caller
maps at every alignment with guarded outputs, the envs' own committed maps after resets, steps and episode ends (SmbVecEnv) and
under a solver budget (SmbReadyVecEnv) against the numpy statement of the rules (tests/measures_numpy.py, T = 7), masked tile
ids, a group sum beyond 32 bits, graph capture and the gym adapter.

Equality: every integer exact; every float form but entropy bit-equal to the reference's recorded answer; entropy bit-equal to
measures_numpy in this process (the same host log built both tables) and within 1e-13 of the recorded one (at most 7 terms below
0.37, each a few ulps of the host's log off, divided by ln 7: an error near 1e-15) -- the convention of
tests/test_gpu_measures.py."""
import glob
import os

import numpy as np
import pytest

import measures_numpy as mn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from conftest import GOLDEN  # noqa: E402

DEV = "cuda:0"
T = 7
POWER = 1000  # the measures are functions of the maps alone: a small search keeps the steps short
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "smb_measures", "*.npz")))
REF_KEYS = (("emptiness", "ref_emptiness"), ("symmetry-horizontal", "ref_sym_hor"), ("symmetry-vertical", "ref_sym_ver"),
            ("symmetry", "ref_sym"), ("co-occurance", "ref_co"))


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
    from control_pcgrl_amd import SmbEvaluator
    return SmbEvaluator(shape, DEV, solver_power=POWER, max_levels=1)


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
    _check_measures(m, grids, fixture_id(path))
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


def test_caller_maps_at_every_alignment_with_guarded_outputs():
    """17 maps of 5 x 7: a map is 35 bytes, so the 17 starts take every value mod 16; the batch itself begins 0, 1, 5 and 9
    bytes into a larger tensor.  The C entry points write into guarded buffers: nothing outside an output is touched."""
    from control_pcgrl_amd import _lib
    L = _lib.lib()
    H, W, n, K = 5, 7, 17, 17
    rng = np.random.default_rng(35)
    grids = rng.integers(0, T, size=(n, H, W), dtype=np.uint8)
    assert {(35 * i) % 16 for i in range(n)} == set(range(16))
    ev = _evaluator((H, W))
    tab = ev._entropy_table()
    results = []
    for start in (0, 1, 5, 9):
        big = torch.full((start + n * H * W + 64,), 6, dtype=torch.uint8, device=DEV)
        view = big[start:start + n * H * W].view(n, H, W)
        view.copy_(torch.as_tensor(grids))
        assert view.data_ptr() % 16 == start
        m = ev.measures(view)
        d = ev.diversity(view, pairwise=True)
        _check_measures(m, grids, f"start {start}")
        _check_diversity(d, grids, K, f"start {start}")
        out = {"counts": Guarded(n * T * 4, torch.int32, (n, T)), "match": Guarded(n * 3 * 4, torch.int32, (n, 3)),
               "forms": Guarded(n * 12 * 8, torch.float64, (n, 12)), "entropy": Guarded(n * 8, torch.float64, (n,)),
               "scratch": Guarded(int(L.pcgrl_smb_diversity_scratch_bytes(H, W, n)), torch.int64, (-1,)),
               "sum": Guarded(8, torch.int64, (1,)), "scores": Guarded(16, torch.float64, (1, 2)),
               "nearest": Guarded(n * 4, torch.int32, (n,)), "nearest_idx": Guarded(n * 4, torch.int32, (n,)),
               "pairwise": Guarded(K * K * 4, torch.int32, (1, K, K))}
        assert out["scratch"].nbytes == n * (3 * 1 + 1) * 8
        stream = torch.cuda.current_stream().cuda_stream
        assert L.pcgrl_smb_measures_for_grids(H, W, n, view.data_ptr(), out["counts"].ptr, out["match"].ptr, out["forms"].ptr,
                                              out["entropy"].ptr, tab.data_ptr(), stream) == 0
        assert L.pcgrl_smb_diversity_for_grids(H, W, n, view.data_ptr(), K, out["scratch"].ptr, out["sum"].ptr,
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
        results.append((m, d))
    for m, d in results[1:]:  # equal to the aligned call
        _same_measures(m, results[0][0])
        _same_diversity(d, results[0][1])
    ev.close()


OWN = [("turtle", (5, 7), None, 110), ("narrow", (16, 116), 0.022, 40)]


@pytest.mark.parametrize("rep,shape,change_percentage,more", OWN, ids=["turtle-5x7", "narrow-16x116"])
def test_measures_and_diversity_of_the_envs_own_maps(rep, shape, change_percentage, more):
    """after reset, after 30 random steps, and across an episode end with auto_reset (5 x 7: after 106 steps; 16 x 116: after
    max_changes = 40 changes)"""
    from control_pcgrl_amd import SmbVecEnv
    n, K = 65, 5
    env = SmbVecEnv(rep, shape, n, device=DEV, seeds=31 + np.arange(n), auto_reset=True, solver_power=POWER,
                    change_percentage=change_percentage)
    env.reset()
    gen = torch.Generator().manual_seed(6)

    def steps(k):
        for _ in range(k):
            env.step(torch.randint(0, env.num_actions, (n,), generator=gen, dtype=torch.int32).to(env.device))

    def check(what):
        grids = env.get_state().grids
        host = _np(grids)
        m = env.measures()
        _check_measures(m, host, what)
        _same_measures(m, env.measures_for_grids(grids))
        assert env.measures(entropy=False).entropy is None
        d = env.diversity(group=K, pairwise=True)
        _check_diversity(d, host, K, what)
        _same_diversity(d, env.diversity_for_grids(grids, group=K, pairwise=True))
        whole = env.diversity()
        _check_diversity(whole, host, n, what + " (one group)")
        return host

    first = check("after reset")
    steps(30)
    assert int(env.last_episode().count.sum()) == 0
    stepped = check("after 30 steps")
    assert not np.array_equal(first, stepped)
    steps(more)
    assert int(env.last_episode().count.min()) >= 1  # every env has drawn a new map inside a step
    ended = check("after an episode end")
    assert not np.array_equal(ended, stepped)
    env.check_errors()
    env.close()


def test_ready_env_shows_the_committed_maps():
    """under a solver budget a busy env's step in flight is not shown: measures() / diversity() are those of
    get_state().grids, while some envs are busy and some idle"""
    from control_pcgrl_amd import SmbReadyVecEnv
    n, K = 65, 5
    env = SmbReadyVecEnv("narrow", (5, 7), n, solver_budget=8, device=DEV, seeds=77 + np.arange(n), auto_reset=True,
                         solver_power=POWER)
    env.reset()
    gen = torch.Generator().manual_seed(8)
    mixed = 0
    for launch in range(40):
        busy = _np(env.env_busy()).astype(bool)
        if busy.any() and not busy.all():
            mixed += 1
            grids = env.get_state().grids
            host = _np(grids)
            _check_measures(env.measures(), host, f"launch {launch}")
            _check_diversity(env.diversity(group=K, pairwise=True), host, K, f"launch {launch}")
            _same_measures(env.measures(), env.measures_for_grids(grids))
            if mixed == 3:
                break
        env.step_ready(torch.randint(0, env.num_actions, (n,), generator=gen, dtype=torch.int32).to(env.device))
    assert mixed >= 1, "no launch left both busy and idle envs behind"
    env.check_errors()
    env.close()


def test_tile_ids_are_masked_to_three_bits():
    """id 7 matches no count but still compares, ids >= 8 alias, and no error bit is set"""
    from control_pcgrl_amd import SmbVecEnv
    rng = np.random.default_rng(7)
    H, W = 5, 7
    raw = rng.integers(0, 256, size=(10, H, W), dtype=np.uint8)
    raw[0], raw[1], raw[2], raw[3] = 7, 8, 255, 0  # all-7, all-8 (= all-0), all-255 (= all-7), all-0
    kept = mn.mask_ids(raw, T)
    assert kept.max() == 7
    ev = _evaluator((H, W))
    env = SmbVecEnv("narrow", (H, W), 2, device=DEV, solver_power=POWER)
    for who in (ev.measures, env.measures_for_grids):
        a, b = who(torch.as_tensor(raw)), who(torch.as_tensor(kept))
        _same_measures(a, b)
        _check_measures(a, raw, "masked")
        assert a.counts[0].tolist() == [0] * 7 and a.counts[2].tolist() == [0] * 7  # id 7 is counted nowhere ...
        assert a.match[0].tolist() == [2 * 7, 5 * 3, 4 * 35]                        # ... and still compares
        assert a.counts[1].tolist() == [35, 0, 0, 0, 0, 0, 0] == a.counts[3].tolist()
        assert float(a.entropy[0]) == 0.0 and int(a.counts.sum(1).min()) < 35
    for who in (ev.diversity, env.diversity_for_grids):
        d = who(torch.as_tensor(raw), group=5, pairwise=True)
        _check_diversity(d, raw, 5, "masked")
        pw = d.pairwise[0]
        assert int(pw[0, 2]) == 0 and int(pw[1, 3]) == 0 and int(pw[0, 1]) == 35  # 7 = 255, 8 = 0, 7 against 0: once a cell
        _same_diversity(d, who(torch.as_tensor(kept), group=5, pairwise=True))
    ev.check_errors()
    env.check_errors()
    env.close()
    ev.close()


def test_sum_beyond_32_bits():
    """2 048 maps of 16 x 128, half all-0 and half all-1, in one group: S = 2 * 1024^2 * 2048 = 2^32"""
    n, H, W = 2048, 16, 128
    grids = torch.zeros((n, H, W), dtype=torch.uint8, device=DEV)
    grids[n // 2:] = 1
    ev = _evaluator((H, W))
    d = ev.diversity(grids)
    S = 2 * 1024 * 1024 * 2048
    assert S == 4294967296 and int(d.hamming_sum[0]) == S
    assert np.array_equal(_bits(_np(d.div_score)), _bits(mn.div_score([S], n, H * W)))
    assert np.array_equal(_bits(_np(d.diversity_bonus)), _bits(mn.diversity_bonus([S], n, H * W)))
    assert int(d.nearest.abs().sum()) == 0  # every map has a copy
    want = np.zeros(n, dtype=np.int32)  # ... the lowest one: 0 (1 for map 0), 1024 (1025 for map 1024)
    want[0], want[n // 2:], want[n // 2] = 1, n // 2, n // 2 + 1
    assert np.array_equal(_np(d.nearest_idx), want)
    m = ev.measures(grids[n // 2 - 2:n // 2 + 2])
    assert m.counts[:, :2].tolist() == [[2048, 0], [2048, 0], [0, 2048], [0, 2048]] and m.match[:, 2].tolist() == [4 * 2048] * 4
    ev.check_errors()
    ev.close()


def test_measures_and_diversity_captured_in_one_graph():
    """one measures() + diversity() pair captured on one side stream and replayed after further steps: the replayed results
    equal fresh calls (the entropy table is uploaded by the eager warm-up, before the capture)"""
    from control_pcgrl_amd import SmbVecEnv
    n, K, shape = 64, 32, (4, 65)
    env = SmbVecEnv("turtle", shape, n, device=DEV, seeds=70 + np.arange(n), auto_reset=True, solver_power=POWER)
    env.reset()
    gen = torch.Generator().manual_seed(72)

    def steps(k):
        for _ in range(k):
            env.step(torch.randint(0, env.num_actions, (n,), generator=gen, dtype=torch.int32).to(env.device))

    steps(3)
    env.measures()
    env.diversity(group=K, pairwise=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            m = env.measures()
            d = env.diversity(group=K, pairwise=True)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for t in range(3):
        steps(8)
        graph.replay()
        host = _np(env.get_state().grids)
        _check_measures(m, host, f"replay {t}")
        _check_diversity(d, host, K, f"replay {t}")
        _same_measures(m, env.measures())
        _same_diversity(d, env.diversity(group=K, pairwise=True))
        seen.append(host)
    assert not np.array_equal(seen[0], seen[-1])  # (the steps did change the maps)
    env.check_errors()
    env.close()


def test_gym_adapter_measures():
    from control_pcgrl_amd import make_env
    env = make_env({"task": {"problem": "smb", "map_shape": (16, 116), "solver_power": POWER}, "representation": "narrow"},
                   device=DEV)
    env.reset(seed=4)
    env.step(1)
    got = env.measures
    g = env.get_map()[None]
    cnt, mat = mn.counts(g, T), mn.matches(g, T)
    want = mn.bc_from_integers(cnt, mat, 16, 116, T)
    assert set(got) == set(mn.BC_NAMES) | {"tile_fractions"}
    for key in mn.BC_NAMES:
        assert isinstance(got[key], float) and got[key] == float(want[key][0]), key
    assert got["tile_fractions"] == mn.tile_fractions(cnt, 16 * 116)[0].tolist()
    row = env._vec.measures()  # the batch form's row
    assert {k: float(v[0]) for k, v in row.bc.items()} == {k: got[k] for k in mn.BC_NAMES}
    assert row.tile_fractions[0].tolist() == got["tile_fractions"]
    env.close()
