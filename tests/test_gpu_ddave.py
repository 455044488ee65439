"""Dangerous Dave levels on the device (control_pcgrl_amd.ddave.DDaveEvaluator, csrc/ddave/pcgrl_ddave.h): the kernel against
the fixtures recorded from the reference (tests/golden/ddave) and against the plain-Python rules (tests/ddave_rules.py) on
generated levels (tests/ddave_levels.py); the reward and the episode end against the reference's recorded values; the measures
and the diversity against tests/measures_numpy.py and the fixtures with T = 7.  Integers are compared exactly, doubles as their
64-bit patterns."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest
import torch

import ddave_levels as DL
import ddave_rules as R
from fixture_cases import fixture_cases
import measures_numpy as mn
from control_pcgrl_amd import _lib
from control_pcgrl_amd.ddave import DDAVE_MEASURE_NAMES, DDaveEvaluator, ddave_config

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ddave")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "dd_*.npz")))
CASES, CASE_IDS = fixture_cases(FILES)  # each file as ever, and split into several launches
MEAS_FILES = sorted(glob.glob(os.path.join(GOLDEN, "meas_*.npz")))
DEV = "cuda:0"
T = 7
# (rows, columns, solver power, levels): every shape at both powers
GENERATED = [(1, 1, 50, 64), (1, 3, 50, 64), (2, 3, 200, 96), (3, 4, 200, 128), (5, 13, 50, 128), (7, 11, 200, 256),
             (16, 32, 50, 64), (1, 1, 200, 64), (1, 3, 200, 64), (2, 3, 50, 96), (3, 4, 50, 128), (5, 13, 200, 128),
             (7, 11, 50, 256), (16, 32, 200, 64)]
CAP = 200  # a returned node is never deeper than the power, 200 at the most here: every generated level's moves fit
REF_KEYS = (("emptiness", "ref_emptiness"), ("symmetry-horizontal", "ref_sym_hor"), ("symmetry-vertical", "ref_sym_ver"),
            ("symmetry", "ref_sym"), ("co-occurance", "ref_co"))


@functools.lru_cache(maxsize=None)
def levels_and_rules(h, w, power, n, cap=CAP):
    """n generated levels (the six generators in turn) and what the rules say about each; computed once per case and shared:
    the tests copy before they change a map."""
    rng = np.random.default_rng(31 + h * 100 + w)
    maps = DL.mixed(rng, h, w, n)
    assert (maps == DL.DIAMOND).reshape(n, -1).sum(1).max() <= 64
    return maps, expect(maps, power, cap)


def expect(maps, power, cap):
    rows = [R.outputs(m, power, cap) for m in maps]
    out = {"stats": np.asarray([r[0] for r in rows], np.int32).reshape(len(maps), 11),
           "length": np.asarray([r[2] for r in rows], np.int32),
           "play": np.asarray([r[3] for r in rows], np.int32).reshape(len(maps), 12),
           "error": np.asarray([int(R.has_error(m)) for m in maps], np.int32)}
    if cap:
        out["moves"] = np.asarray([r[1] for r in rows], np.int8).reshape(len(maps), cap)
    out["won"] = (out["play"][:, 0] >= 1) & (out["play"][:, 0] <= 4)
    return out


def cut(want, lo, hi, cap=None):
    out = {k: v[lo:hi] for k, v in want.items()}
    if cap is not None:
        moves = out.pop("moves")
        if cap:
            out["moves"] = np.concatenate([moves, np.full((len(moves), max(0, cap - moves.shape[1])), -1, np.int8)], 1)[:, :cap]
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _np(t):
    return t.cpu().numpy()


def assert_same(got, want, what=""):
    assert set(got) == set(want), (set(got), set(want))
    for k in want:
        g = _np(got[k]) if isinstance(got[k], torch.Tensor) else got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape, want[k].dtype, want[k].shape)
        bad = np.nonzero((g != want[k]).reshape(len(g), -1).any(axis=1))[0]
        assert bad.size == 0, (what, k, "levels", bad[:8].tolist(), g[bad[0]].tolist(), want[k][bad[0]].tolist())


@pytest.mark.parametrize("path,max_levels", CASES, ids=CASE_IDS)
def test_kernel_equals_fixtures(path, max_levels):
    z = np.load(path)
    grids, power = z["grids"], int(z["power"])
    n, cap = len(grids), z["moves"].shape[1]
    status = z["play"][:, 0]
    want = {"stats": z["stats"], "moves": z["moves"], "length": z["length"], "play": z["play"], "error": np.zeros(n, np.int32),
            "won": (status >= 1) & (status <= 4)}
    # the record says what the reference's getSolution calls returned
    ran = z["stage_won"] >= 0
    assert np.array_equal(np.where(ran, z["stage_iters"], 0), z["play"][:, 1:5])
    assert np.array_equal((z["stage_won"] == 1).any(1), want["won"])
    with DDaveEvaluator(grids.shape[1:], DEV, solver_power=power, max_levels=max_levels or 256) as ev:
        assert_same(ev.evaluate(grids, move_cap=cap), want, os.path.basename(path))
        ev.check_errors()
        # the reward and the episode end of the recorded pairs, bit for bit
        new, old = torch.from_numpy(z["rew_new"]).to(DEV), torch.from_numpy(z["rew_old"]).to(DEV)
        rew = ev.reward(new, old)
        assert rew.dtype == torch.float64 and np.array_equal(bits(_np(rew)), z["rew_bits"])
        over = ev.episode_over(new)
        assert over.dtype == torch.bool and np.array_equal(_np(over), z["over"])
    weights = dict(zip(R.REWARD_ORDER, z["custom_weights"].tolist()))
    md, ms, tj, ts = (int(v) for v in z["custom_params"])
    with DDaveEvaluator(grids.shape[1:], DEV, solver_power=power, weights=weights, max_diamonds=md, min_spikes=ms,
                        target_jumps=tj, target_solution=ts, max_levels=1) as ev:
        assert np.array_equal(bits(_np(ev.reward(new, old))), z["rew_bits_custom"])
        assert np.array_equal(_np(ev.episode_over(new)), z["over_custom"])
    assert (z["rew_bits_custom"] != z["rew_bits"]).any()


@pytest.mark.parametrize("h,w,power,n", GENERATED, ids=[f"{h}x{w}-p{p}" for h, w, p, _ in GENERATED])
def test_kernel_equals_rules_on_generated_levels(h, w, power, n):
    maps, want = levels_and_rules(h, w, power, n)
    with DDaveEvaluator((h, w), DEV, solver_power=power, max_levels=256) as ev:
        assert_same(ev.evaluate(maps, move_cap=CAP), want, f"{h}x{w} power {power}")
        ev.check_errors()
    assert (want["play"][:, 0] != 5).all()  # no case is skipped: the generators never exceed 64 diamonds
    if h * w >= 12:
        assert (want["play"][:, 0] >= 0).sum() >= n // 4  # and a good share of the levels reaches the solver


def test_a_level_with_65_diamonds_is_not_searched():
    m = np.full((8, 11), DL.DIAMOND, np.uint8)
    m[7] = DL.SOLID
    m[6, :3] = (DL.PLAYER, DL.KEY, DL.EXIT)
    m[0, :9] = DL.EMPTY
    fewer = m.copy()
    fewer[0, 9] = DL.EMPTY
    assert (m == DL.DIAMOND).sum() == 65 and (fewer == DL.DIAMOND).sum() == 64
    maps = np.stack([m, fewer])
    want = expect(maps, 50, 8)
    assert want["play"][0].tolist() == [5] + [0] * 9 + [65, 0] and want["stats"][0].tolist() == [1, 0, 1, 65, 1, 0, 1, 0, 0, 88, 0]
    assert want["play"][1, 0] == 1 and (want["moves"][0] == -1).all()
    with DDaveEvaluator((8, 11), DEV, solver_power=50, max_levels=2) as ev:
        assert_same(ev.evaluate(maps, move_cap=8), want)
        ev.check_errors()  # no error bit


def test_move_cap_zero_three_and_above_the_length():
    maps, want = levels_and_rules(7, 11, 200, 256)
    assert 3 < want["length"].max() <= CAP
    with DDaveEvaluator((7, 11), DEV, solver_power=200, max_levels=256) as ev:
        none = ev.evaluate(maps)
        assert "moves" not in none
        assert_same(none, cut(want, 0, 256, 0))
        assert_same(ev.evaluate(maps, move_cap=3), cut(want, 0, 256, 3))  # `length` stays complete
        assert_same(ev.evaluate(maps, move_cap=CAP + 60), cut(want, 0, 256, CAP + 60))


def test_null_outputs_stay_untouched():
    """through the C ABI: with move_cap = 0 the move buffer is not written even when given, and with every optional output
    null only the statistics are"""
    maps, want = levels_and_rules(7, 11, 200, 256)
    n = 70
    L = _lib.lib()
    g = torch.from_numpy(maps[:n].copy()).to(DEV)
    nbytes = L.pcgrl_ddave_workspace_bytes(n, 7, 11, 200)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    guard = 16
    stats = torch.full((n * 11 + 2 * guard,), 99, dtype=torch.int32, device=DEV)
    moves = torch.full((n * CAP + 2 * guard,), 77, dtype=torch.int8, device=DEV)
    length = torch.full((n + 2 * guard,), 55, dtype=torch.int32, device=DEV)
    play = torch.full((n * 12 + 2 * guard,), 33, dtype=torch.int32, device=DEV)
    cfg = ddave_config((7, 11), 200)
    stream = torch.cuda.current_stream().cuda_stream

    def ptr(t):
        return t[guard:].data_ptr()

    def call(cap, mv, ln, pl):
        _lib.check(L.pcgrl_ddave_evaluate(C.byref(cfg), n, g.data_ptr(), ws.data_ptr(), nbytes, cap, ptr(stats), mv, ln, pl,
                                          None, stream))
        torch.cuda.synchronize()

    call(0, ptr(moves), None, None)
    assert np.array_equal(_np(stats[guard:-guard]).reshape(n, 11), want["stats"][:n])
    assert (stats[:guard] == 99).all() and (stats[-guard:] == 99).all()
    assert (moves == 77).all() and (length == 55).all() and (play == 33).all()
    call(CAP, ptr(moves), None, ptr(play))
    assert np.array_equal(_np(moves[guard:-guard]).reshape(n, CAP), want["moves"][:n])
    assert np.array_equal(_np(play[guard:-guard]).reshape(n, 12), want["play"][:n])
    for t, v in ((moves, 77), (play, 33)):
        assert (t[:guard] == v).all() and (t[-guard:] == v).all()
    assert (length == 55).all()
    moves.fill_(77)
    call(CAP, None, ptr(length), None)
    assert np.array_equal(_np(length[guard:-guard]), want["length"][:n]) and (moves == 77).all()
    assert (length[:guard] == 55).all() and (length[-guard:] == 55).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(n):
    maps, want = levels_and_rules(7, 11, 200, 256)
    with DDaveEvaluator((7, 11), DEV, solver_power=200, max_levels=128) as ev:
        assert_same(ev.evaluate(maps[:n], move_cap=CAP), cut(want, 0, n), f"n={n}")


def test_batches_above_max_levels_run_as_successive_launches():
    maps, want = levels_and_rules(7, 11, 200, 256)
    with DDaveEvaluator((7, 11), DEV, solver_power=200, max_levels=3) as ev:
        assert_same(ev.evaluate(maps[:20], move_cap=CAP), cut(want, 0, 20))


@pytest.mark.parametrize("h,w,power,n", [(7, 11, 200, 256), (5, 13, 50, 128), (16, 32, 50, 64)], ids=["7x11", "5x13", "16x32"])
def test_unaligned_grid_pointers(h, w, power, n):
    maps, want = levels_and_rules(h, w, power, n)
    n = 40
    with DDaveEvaluator((h, w), DEV, solver_power=power, max_levels=64) as ev:
        for off in (1, 3, 8, 15):
            buf = torch.zeros(n * h * w + 16, dtype=torch.uint8, device=DEV)
            g = buf[off:off + n * h * w].view(n, h, w)
            g.copy_(torch.from_numpy(maps[:n].copy()))
            assert g.data_ptr() % 16 == (buf.data_ptr() + off) % 16
            assert_same(ev.evaluate(g, move_cap=CAP), cut(want, 0, n), f"offset {off}")
            assert np.array_equal(_np(ev.measures(g).counts), mn.counts(maps[:n], T)), off


def test_a_dirty_workspace_gives_the_same_results():
    """nodes and heap are written before they are read and the tags are cleared before each stage: a workspace of 0xFF bytes
    changes nothing"""
    maps, want = levels_and_rules(7, 11, 200, 256)
    with DDaveEvaluator((7, 11), DEV, solver_power=200, max_levels=256) as ev:
        ev._workspace.fill_(-1)
        assert_same(ev.evaluate(maps, move_cap=CAP), want, "dirty")
        ev._workspace.fill_(-1)
        assert_same(ev.evaluate(maps[:65], move_cap=CAP), cut(want, 0, 65), "dirty, again")


def test_tile_ids_above_6_read_as_solid_and_set_the_error_bit():
    maps, _ = levels_and_rules(7, 11, 200, 256)
    dirty = maps[:16].copy()
    dirty[5, 3, 4] = 7
    dirty[9, 0, 0] = 255
    dirty[9, 6, 10] = 8
    want = expect(dirty, 200, CAP)  # (the rules read them as solid too)
    assert want["error"].tolist() == [int(i in (5, 9)) for i in range(16)]
    clean = dirty.copy()
    clean[clean > 6] = DL.SOLID
    assert np.array_equal(expect(clean, 200, CAP)["stats"], want["stats"])
    with DDaveEvaluator((7, 11), DEV, solver_power=200, max_levels=16) as ev:
        assert_same(ev.evaluate(dirty, move_cap=CAP), want)  # the rest of the batch is unaffected
        with pytest.raises(ValueError):
            ev.check_errors()
        ev.check_errors()  # cleared: raises once


def test_custom_weights_and_targets():
    maps, want = levels_and_rules(7, 11, 200, 256)
    stats = want["stats"]
    new, old = stats[:128], stats[128:]
    w = {"player": 0.5, "dist-win": 0.3, "regions": 2.25, "spikes": 0.0}
    with DDaveEvaluator((7, 11), DEV, solver_power=200, weights=w, max_diamonds=1, min_spikes=4, target_jumps=0,
                        target_solution=6, max_levels=1) as ev:
        rew = _np(ev.reward(torch.from_numpy(new).to(DEV), torch.from_numpy(old).to(DEV)))
        mine = np.asarray([float(R.reward(a, b, w, 1, 4)) for a, b in zip(new, old)])
        assert np.array_equal(bits(rew), bits(mine))
        over = _np(ev.episode_over(torch.from_numpy(stats).to(DEV)))
        assert over.tolist() == [R.episode_over(s, 0, 6) for s in stats] and over.any() and not over.all()
    stock = np.asarray([float(R.reward(a, b)) for a, b in zip(new, old)])
    assert (stock != mine).any()
    with pytest.raises(ValueError):
        DDaveEvaluator((7, 11), DEV, weights={"col-diamonds": 1})


@pytest.mark.parametrize("path", MEAS_FILES, ids=[os.path.basename(f)[:-4] for f in MEAS_FILES])
def test_measures_and_diversity_equal_fixtures(path):
    z = np.load(path)
    grids = z["grids"]
    h, w = grids.shape[1:]
    with DDaveEvaluator((h, w), DEV, solver_power=1, max_levels=1) as ev:
        m = ev.measures(grids)
        assert np.array_equal(_np(m.counts), z["counts"]) and np.array_equal(_np(m.match), z["match"])
        for key, name in REF_KEYS:  # the reference's own answers, bit for bit
            assert np.array_equal(bits(_np(m.bc[key])), bits(z[name])), key
        assert np.array_equal(bits(_np(m.tile_fractions)), bits(z["ref_tile_fractions"]))
        assert np.abs(_np(m.entropy) - z["ref_entropy"]).max() <= 1e-13  # (the table is built with this host's log)
        gi = 0
        for c in range(len(z["div_K"])):
            K, G = int(z["div_K"][c]), int(z["div_G"][c])
            lo, hi = int(z["div_off"][c]), int(z["div_off"][c + 1])
            d = ev.diversity(grids[z["div_idx"][lo:hi]], group=K)
            assert np.array_equal(_np(d.hamming_sum), z["div_sum"][gi:gi + G]), (K, G)
            assert np.array_equal(_np(d.nearest), z["div_nearest"][lo:hi]), (K, G)
            assert np.array_equal(_np(d.nearest_idx), z["div_nearest_idx"][lo:hi]), (K, G)
            assert np.array_equal(bits(_np(d.div_score)), bits(z["div_ref_score"][gi:gi + G])), (K, G)
            assert np.array_equal(bits(_np(d.diversity_bonus)), bits(z["div_ref_bonus"][gi:gi + G])), (K, G)
            gi += G


@pytest.mark.parametrize("h,w,power,n", [(5, 13, 50, 128), (16, 32, 50, 64)], ids=["5x13", "16x32"])
def test_measures_and_diversity_against_the_numpy_rules(h, w, power, n):
    maps, _ = levels_and_rules(h, w, power, n)
    with DDaveEvaluator((h, w), DEV, solver_power=1, max_levels=1) as ev:
        m = ev.measures(maps)
        cnt, mat = mn.counts(maps, T), mn.matches(maps, T)
        assert m.counts.dtype == torch.int32 and tuple(m.counts.shape) == (n, T) and tuple(m.forms.shape) == (n, 5 + T)
        assert np.array_equal(_np(m.counts), cnt) and np.array_equal(_np(m.match), mat)
        bc = mn.bc_from_integers(cnt, mat, h, w, T)
        assert set(m.bc) == set(mn.BC_NAMES) == set(DDAVE_MEASURE_NAMES)
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
        ev.check_errors()


def test_behaviour_vectors():
    maps, want = levels_and_rules(7, 11, 200, 256)
    with DDaveEvaluator((7, 11), DEV, solver_power=200, max_levels=256) as ev:
        meas = ev.measures(maps)
        b = ev.behaviour(maps, ("emptiness", "sol-length", "dist-win"))
        assert b.dtype == torch.float64 and tuple(b.shape) == (len(maps), 3)
        assert torch.equal(b[:, 0], meas.bc["emptiness"])
        assert np.array_equal(_np(b[:, 1]), want["stats"][:, 10].astype(np.float64))
        assert np.array_equal(_np(b[:, 2]), want["stats"][:, 9].astype(np.float64))
        assert (_np(ev.behaviour(maps, "NONE")) == 0).all() and tuple(ev.behaviour(maps, "NONE").shape) == (len(maps), 1)
        # only what the names need is launched
        calls = []
        real = ev.measures
        ev.measures = lambda *a, **k: calls.append("measures")
        assert np.array_equal(_np(ev.behaviour(maps, ("num-jumps", "NONE"))[:, 0]), want["stats"][:, 7].astype(np.float64))
        assert not calls
        ev.measures = real
        ev.evaluate = lambda *a, **k: calls.append("evaluate")
        assert torch.equal(ev.behaviour(maps, ("entropy", "NONE"))[:, 0], meas.bc["entropy"]) and not calls
        with pytest.raises(ValueError):
            ev.behaviour(maps, ("path-length",))


def test_evaluate_under_graph_capture():
    maps, want = levels_and_rules(7, 11, 200, 256)
    static = torch.from_numpy(maps[:96].copy()).to(DEV)
    with DDaveEvaluator((7, 11), DEV, solver_power=200, max_levels=64) as ev:
        eager = {k: v.clone() for k, v in ev.evaluate(static, move_cap=CAP).items()}
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            ev.evaluate(static, move_cap=CAP)
        torch.cuda.current_stream(DEV).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = ev.evaluate(static, move_cap=CAP)
        for k in ("stats", "moves", "length", "play", "error"):
            captured[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            if k != "won":  # (derived from `play` when evaluate() returned: not part of the graph's outputs)
                assert torch.equal(captured[k], eager[k]), k
        captured["won"] = (captured["play"][:, 0] >= 1) & (captured["play"][:, 0] <= 4)
        assert_same(captured, cut(want, 0, 96))
        # replayed on changed input
        static.copy_(torch.from_numpy(maps[96:192].copy()))
        graph.replay()
        torch.cuda.synchronize()
        captured["won"] = (captured["play"][:, 0] >= 1) & (captured["play"][:, 0] <= 4)
        assert_same(captured, cut(want, 96, 192))
        ev.check_errors()
