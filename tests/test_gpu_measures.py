"""Level measures and pairwise Hamming diversity (include/pcgrl_amd_measures.h) on the GPU: every fixture recorded from the
reference (tests/golden/measures/, tools/gen_golden_measures.py) through measures_for_grids / diversity_for_grids, the
engine's own maps after resets / steps / updates against the numpy statement of the rules (tests/measures_numpy.py) on one
engine and on sub-batches, the pairwise matrix, a sum beyond 32 bits, graph capture, masked tile ids and the refusals.

Equality: every integer exact; every float form but entropy bit-equal to the reference's recorded answer; entropy bit-equal to
measures_numpy in this process (the same host log built both tables) and within 1e-13 of the recorded one (at most 8 terms
below 0.37, each a few ulps of the host's log off, divided by at least ln 2: an error near 1e-15)."""
import glob
import math
import os

import numpy as np
import pytest

import measures_numpy as mn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from conftest import GOLDEN  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "measures", "*.npz")))
REF_KEYS = (("emptiness", "ref_emptiness"), ("symmetry-horizontal", "ref_sym_hor"), ("symmetry-vertical", "ref_sym_ver"),
            ("symmetry", "ref_sym"), ("co-occurance", "ref_co"))


def fixture_id(path):
    return os.path.basename(path)[:-4]


def _vec(*a, **k):
    from control_pcgrl_amd import VecPcgrlEnv
    return VecPcgrlEnv(*a, **k)


def _env_for(problem, shape, n=4, rep="narrow", **kw):
    """an engine for `shape` (zelda's static nearest-enemy target range is empty on a 1 x 1 or 1 x 5 map and the engine refuses
    that config, as the reference's loss fails on it: the measures are functions of the map alone, so those shapes get a
    range of their own)"""
    if problem == "zelda" and math.ceil(shape[1] / 2 + 1) * shape[0] <= 5:
        kw["static_trgs"] = {"nearest-enemy": (0, 1)}
    return _vec(problem, rep, shape, n, **kw)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _check_measures(m, grids, T, what):
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
    return bc


def _check_diversity(d, grids, T, K, what, want=None):
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


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_fixtures_through_measures_for_grids(path):
    z = np.load(path)
    problem, shape = fixture_id(path).split("_")
    H, W = (int(v) for v in shape.split("x"))
    T = mn.N_TILES[problem]
    env = _env_for(problem, (H, W))
    grids = z["grids"]
    m = env.measures_for_grids(torch.as_tensor(grids))
    assert np.array_equal(_np(m.counts), z["counts"]) and np.array_equal(_np(m.match), z["match"])
    _check_measures(m, grids, T, fixture_id(path))
    for key, name in REF_KEYS:  # the reference's own answers, bit for bit
        assert np.array_equal(_bits(_np(m.bc[key])), _bits(z[name])), key
    assert np.array_equal(_bits(_np(m.tile_fractions)), _bits(z["ref_tile_fractions"]))
    err = np.abs(_np(m.entropy) - z["ref_entropy"]).max()
    print(f"{fixture_id(path)}: entropy differs from the recorded one by at most {err:.3e}")
    assert err <= 1e-13
    # without entropy: the same integers, no table
    m2 = env.measures_for_grids(torch.as_tensor(grids), entropy=False)
    assert m2.entropy is None and "entropy" not in m2.bc
    assert torch.equal(m2.counts, m.counts) and torch.equal(m2.match, m.match)
    # a single map and no maps
    one = env.measures_for_grids(torch.as_tensor(grids[-1:]))
    assert torch.equal(one.counts, m.counts[-1:]) and torch.equal(one.match, m.match[-1:])
    none = env.measures_for_grids(torch.empty((0, H, W), dtype=torch.uint8))
    assert tuple(none.counts.shape) == (0, T) and tuple(none.bc["symmetry"].shape) == (0,)
    env.check_errors()
    env.close()


@pytest.mark.parametrize("path", FIXTURES, ids=fixture_id)
def test_fixtures_through_diversity_for_grids(path):
    z = np.load(path)
    problem, shape = fixture_id(path).split("_")
    H, W = (int(v) for v in shape.split("x"))
    T = mn.N_TILES[problem]
    env = _env_for(problem, (H, W))
    gi = 0
    for c in range(len(z["div_K"])):
        K, G = int(z["div_K"][c]), int(z["div_G"][c])
        lo, hi = int(z["div_off"][c]), int(z["div_off"][c + 1])
        sel = z["grids"][z["div_idx"][lo:hi]]
        what = f"{fixture_id(path)} K={K} G={G}"
        d = env.diversity_for_grids(torch.as_tensor(sel), group=K, pairwise=True)
        want = (z["div_sum"][gi:gi + G], z["div_nearest"][lo:hi], z["div_nearest_idx"][lo:hi])
        _check_diversity(d, sel, T, K, what, want=want)
        # the reference's own answers, bit for bit
        assert np.array_equal(_bits(_np(d.div_score)), _bits(z["div_ref_score"][gi:gi + G])), what
        assert np.array_equal(_bits(_np(d.diversity_bonus)), _bits(z["div_ref_bonus"][gi:gi + G])), what
        # the matrix: symmetric, zero diagonal, and it is what the sums and the nearest maps come from
        pw = d.pairwise
        assert tuple(pw.shape) == (G, K, K) and pw.dtype == torch.int32
        assert torch.equal(pw, pw.transpose(1, 2)) and int(pw.diagonal(dim1=1, dim2=2).abs().sum()) == 0
        assert torch.equal(pw.sum((1, 2), dtype=torch.int64), d.hamming_sum)
        off = pw + torch.eye(K, dtype=torch.int32, device=pw.device)[None] * (H * W + 1)
        assert torch.equal(off.min(2).values.reshape(-1), d.nearest), what
        assert torch.equal(torch.gather(pw, 2, d.nearest_idx.view(G, K, 1).long()).reshape(-1), d.nearest), what
        if G == 1:  # group=None is one group of everything
            whole = env.diversity_for_grids(torch.as_tensor(sel))
            assert whole.pairwise is None and torch.equal(whole.hamming_sum, d.hamming_sum)
            assert torch.equal(whole.nearest, d.nearest) and torch.equal(whole.nearest_idx, d.nearest_idx)
        gi += G
    env.check_errors()
    env.close()


OWN = [("binary", "narrow", (16, 16)), ("zelda", "turtle", (16, 16)), ("sokoban", "wide", (16, 16)), ("binary", "turtle", (12, 40)),
       ("zelda", "narrow", (7, 11)), ("sokoban", "narrow", (5, 40)), ("binary", "narrow", (64, 64))]


@pytest.mark.parametrize("problem,rep,shape", OWN, ids=[f"{p}-{r}-{s[0]}x{s[1]}" for p, r, s in OWN])
def test_measures_and_diversity_of_the_engines_own_maps(problem, rep, shape):
    n, K = 130, 65
    T = mn.N_TILES[problem]
    env = _env_for(problem, shape, n=n, rep=rep, seeds=11 + np.arange(n), auto_reset=True)
    env.reset()
    gen = torch.Generator().manual_seed(5)

    def check(what):
        grids = env.get_state().grids
        host = _np(grids)
        m = env.measures()
        _check_measures(m, host, T, what)
        again = env.measures_for_grids(grids)
        assert torch.equal(m.counts, again.counts) and torch.equal(m.match, again.match) and torch.equal(m.entropy, again.entropy)
        d = env.diversity(group=K, pairwise=True)
        _check_diversity(d, host, T, K, what)
        whole = env.diversity()
        _check_diversity(whole, host, T, n, what + " (one group)")
        return host

    first = check("after reset")
    for _ in range(12):
        env.step(torch.randint(0, env.num_actions, (n,), generator=gen, dtype=torch.int32).to(env.device))
    stepped = check("after 12 steps")
    assert not np.array_equal(first, stepped)
    # stale statistics do not matter: maps edited by update(), nothing refreshed
    for _ in range(4):
        env.update(torch.randint(0, env.num_actions, (n,), generator=gen, dtype=torch.int32).to(env.device), want_obs=False)
    stale = check("after update without refresh_stats")
    assert not np.array_equal(stale, stepped)
    env.refresh_stats()
    check("after refresh_stats")
    env.check_errors()
    env.close()


@pytest.mark.parametrize("problem,rep,shape", [("binary", "narrow", (16, 16)), ("zelda", "turtle", (12, 40))])
def test_sub_batched_measures_equal_the_single_engine(problem, rep, shape):
    from control_pcgrl_amd import SubBatchedVecEnv
    n = 64
    T = mn.N_TILES[problem]
    seeds = 9 + np.arange(n)
    one = _vec(problem, rep, shape, n, seeds=seeds)
    four = SubBatchedVecEnv(problem, rep, shape, n, sub_batches=4, seeds=seeds)
    one.reset()
    four.reset()
    gen = torch.Generator().manual_seed(2)
    for _ in range(5):
        a = torch.randint(0, one.num_actions, (n,), generator=gen, dtype=torch.int32).cuda()
        one.step(a)
        four.step(a)
    grids = four.get_state().grids
    assert torch.equal(one.get_state().grids, grids)
    a, b = one.measures(), four.measures()
    _check_measures(b, _np(grids), T, "sub-batched")
    assert torch.equal(a.counts, b.counts) and torch.equal(a.match, b.match) and torch.equal(a.entropy, b.entropy)
    assert four.measures(entropy=False).entropy is None
    with pytest.raises(NotImplementedError, match="straddle"):
        four.diversity(group=16)
    # ... what the message says to do instead
    d = four.envs[0].diversity_for_grids(grids, group=32)
    _check_diversity(d, _np(grids), T, 32, "gathered")
    one.close()
    four.close()


def test_sum_beyond_32_bits():
    """2 048 random binary 64 x 64 maps in one group: S is about 8.6e9, beyond int32 and uint32; the expected value by the
    per-cell histogram identity in int64"""
    rng = np.random.default_rng(2048)
    grids = rng.integers(0, 2, size=(2048, 64, 64), dtype=np.uint8)
    want = mn.hamming_sum(grids, 2)
    assert want > 2 ** 32
    env = _vec("binary", "narrow", (64, 64), 4)
    d = env.diversity_for_grids(torch.as_tensor(grids))
    assert int(d.hamming_sum[0]) == want
    assert np.array_equal(_bits(_np(d.div_score)), _bits(mn.div_score([want], 2048, 4096)))
    # a few rows of the nearest maps by brute force
    flat = grids.reshape(2048, -1)
    for i in (0, 63, 64, 1000, 2047):
        dist = (flat != flat[i]).sum(1)
        dist[i] = 1 << 20
        assert int(d.nearest[i]) == dist.min() and int(d.nearest_idx[i]) == int(dist.argmin())
    env.check_errors()
    env.close()


@pytest.mark.parametrize("problem,shape", [("binary", (16, 16)), ("zelda", (12, 40))])
def test_measures_and_diversity_captured_in_one_graph(problem, shape):
    """"HIP-graph capturable": a step, the measures and the diversity of the stepped maps as one captured chain, replayed with
    fresh actions (the entropy table is uploaded by the eager warm-up, before the capture)"""
    n, K = 64, 32
    T = mn.N_TILES[problem]
    env = _vec(problem, "narrow", shape, n, seeds=70 + np.arange(n), auto_reset=True)
    env.reset()
    gen = torch.Generator().manual_seed(72)
    static_a = torch.zeros(n, dtype=torch.int32, device=env.device)
    for _ in range(3):
        env.step(torch.randint(0, env.num_actions, (n,), generator=gen, dtype=torch.int32).to(env.device))
        env.measures()
        env.diversity(group=K, pairwise=True)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            env.step(static_a)
            m = env.measures()
            d = env.diversity(group=K, pairwise=True)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for t in range(4):
        static_a.copy_(torch.randint(0, env.num_actions, (n,), generator=gen, dtype=torch.int32))
        graph.replay()
        host = _np(env.get_state().grids)
        _check_measures(m, host, T, f"replay {t}")
        _check_diversity(d, host, T, K, f"replay {t}")
        seen.append(host)
    assert not np.array_equal(seen[0], seen[-1])  # (the replays did step)
    env.check_errors()
    env.close()


def test_tile_ids_beyond_the_problem_are_masked():
    """the header: ids are masked to the ceil(log2 T) bits the engine keeps of a tile"""
    rng = np.random.default_rng(4)
    raw = rng.integers(0, 256, size=(10, 7, 11), dtype=np.uint8)
    for problem in ("binary", "sokoban", "zelda"):
        T = mn.N_TILES[problem]
        env = _env_for(problem, (7, 11))
        kept = mn.mask_ids(raw, T)
        a, b = env.measures_for_grids(torch.as_tensor(raw)), env.measures_for_grids(torch.as_tensor(kept))
        assert torch.equal(a.counts, b.counts) and torch.equal(a.match, b.match)
        _check_measures(a, raw, T, problem)
        d = env.diversity_for_grids(torch.as_tensor(raw), group=5, pairwise=True)
        _check_diversity(d, raw, T, 5, problem)
        if problem == "sokoban":  # ids 5..7 are no tile of the problem: counted nowhere, still compared
            assert int(a.counts.sum(1).min()) < 77
        env.close()


def test_refusals():
    env = _vec("minecraft_3D_maze", "narrow", (7, 7, 7), 8)
    env.reset()
    assert env._L.pcgrl_measures_tiles(env._h) == 0 and env._L.pcgrl_diversity_scratch_bytes(env._h, 8) == 0
    with pytest.raises(NotImplementedError, match="get_counts reads an attribute"):
        env.measures()
    with pytest.raises(NotImplementedError, match="2-D problems only"):
        env.diversity()
    with pytest.raises(NotImplementedError, match="pcgrl_measures"):
        env.measures_for_grids(env.get_state().grids)
    env.close()
    env = _vec("binary", "narrow", (16, 16), 12)
    env.reset()
    assert env._L.pcgrl_measures_tiles(env._h) == 2 and env._L.pcgrl_diversity_scratch_bytes(env._h, 12) == 12 * (4 + 1) * 8
    for group in (1, 0, 5, 24):
        with pytest.raises(ValueError, match="group"):
            env.diversity(group=group)
    L, h = env._L, env._h
    buf = torch.zeros(4096, dtype=torch.int64, device=env.device)
    p = buf.data_ptr()
    for rc in (L.pcgrl_measures(h, None, p, None, None, None, None), L.pcgrl_measures(h, p, None, None, None, None, None),
               L.pcgrl_measures(h, p, p, None, p, None, None)):  # (entropy without its table)
        assert rc == 1 and b"pcgrl_measures:" in L.pcgrl_last_error()
    for rc in (L.pcgrl_diversity(h, 5, p, p, None, None, None, None, None), L.pcgrl_diversity(h, 1, p, p, None, None, None, None, None),
               L.pcgrl_diversity(h, 4, None, p, None, None, None, None, None),
               L.pcgrl_diversity(h, 4, p + 4, p, None, None, None, None, None),
               L.pcgrl_diversity(h, 4, p, None, None, None, None, None, None)):
        assert rc == 1 and b"pcgrl_diversity:" in L.pcgrl_last_error()
    assert L.pcgrl_diversity_for_grids(h, 8, None, 4, p, p, None, None, None, None, None) == 1
    assert L.pcgrl_diversity_for_grids(h, 0, None, 4, None, None, None, None, None, None, None) == 0  # (no maps: a no-op)
    assert L.pcgrl_measures_for_grids(h, 0, None, None, None, None, None, None, None) == 0
    # the optional outputs may be left out
    sums = torch.empty(3, dtype=torch.int64, device=env.device)
    assert L.pcgrl_diversity(h, 4, p, sums.data_ptr(), None, None, None, None, None) == 0
    assert torch.equal(sums, env.diversity(group=4).hamming_sum)
    env.check_errors()
    env.close()
    from control_pcgrl_amd.multiagent import MultiAgentVecEnv
    ma = MultiAgentVecEnv("binary", (16, 16), 8, n_agents=2)
    for call in (ma.measures, ma.diversity):
        with pytest.raises(NotImplementedError, match="single-agent"):
            call()
    ma.close()


def test_gym_adapter_measures():
    from control_pcgrl_amd import make_env
    env = make_env({"task": {"problem": "zelda", "map_shape": (16, 16)}, "representation": "narrow"})
    env.reset(seed=4)
    env.step(1)
    got = env.measures
    g = env.get_map()[None]
    cnt, mat = mn.counts(g, 8), mn.matches(g, 8)
    want = mn.bc_from_integers(cnt, mat, 16, 16, 8)
    assert set(got) == set(mn.BC_NAMES) | {"tile_fractions"}
    for key in mn.BC_NAMES:
        assert isinstance(got[key], float) and got[key] == float(want[key][0]), key
    assert got["tile_fractions"] == mn.tile_fractions(cnt, 256)[0].tolist()
    env.close()
