"""Super Mario Bros levels on the device (control_pcgrl_amd.smb.SmbEvaluator, csrc/smb/pcgrl_smb.h): the kernel against the
fixtures recorded from the reference (tests/golden/smb) and against the plain-Python rules (tests/smb_rules.py) on generated
levels (tests/smb_levels.py).  Everything is integers but the loss, which is compared exactly too."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

from fixture_cases import fixture_cases
import smb_levels as SL
import smb_rules as R
from control_pcgrl_amd.smb import SmbEvaluator

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smb")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))
CASES, CASE_IDS = fixture_cases(FILES)  # each file as ever, and split into several launches
DEV = "cuda:0"
SHAPES = [(16, 116), (16, 128), (16, 64), (16, 65), (4, 1), (5, 7), (16, 24)]  # 64 | 65: one | two columns per lane


@functools.lru_cache(maxsize=None)
def levels_and_rules(h, w, power, n=64, seed=1):
    """n generated maps of every kind and what the rules say about each; computed once per (shape, power) and shared: the
    tests copy before they change a map."""
    maps = SL.batch(seed, n, h, w)
    return maps, tuple(R.get_stats(m, power) for m in maps)


def expect(answers, cap, jump_cap):
    """The evaluator's outputs, as the rules give them."""
    n = len(answers)
    out = {"stats": np.zeros((n, 9), np.int32), "loss": np.zeros(n), "won": np.zeros(n, bool), "play": np.zeros((n, 6), np.int32),
           "moves": np.full((n, cap), -1, np.int8), "length": np.zeros(n, np.int32),
           "jump_locs": np.full((n, jump_cap, 2), -1, np.int16)}
    for i, (stats, rec) in enumerate(answers):
        out["stats"][i] = stats
        out["loss"][i] = R.loss(stats)
        out["won"][i] = bool(rec["won"])
        out["play"][i] = [rec["won"], rec["x"], rec["y"], rec["air"], rec["it1"], rec["it2"]]
        k = min(cap, len(rec["moves"]))
        out["moves"][i, :k] = rec["moves"][:k]
        out["length"][i] = len(rec["moves"])
        j = min(jump_cap, len(rec["jump_locs"]))
        if j:
            out["jump_locs"][i, :j] = rec["jump_locs"][:j]
    return out


def assert_same(got, want, what=""):
    assert set(got) == set(want)
    for k in want:
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape)
        bad = np.nonzero((g != want[k]).reshape(len(g), -1).any(axis=1))[0]
        assert bad.size == 0, (what, k, "levels", bad[:8].tolist(), g[bad[0]].tolist(), want[k][bad[0]].tolist())


@pytest.mark.parametrize("path,max_levels", CASES, ids=CASE_IDS)
def test_kernel_equals_fixtures(path, max_levels):
    z = np.load(path)
    grids, power = z["grids"], int(z["solver_power"])
    n = len(grids)
    final = np.where(z["p1_won"] != 0, 1, 2)  # the play-through get_stats reports: pass 1's when it wins, else pass 2's

    def pick(field):
        return [z[f"p{final[i]}_{field}"][i] for i in range(n)]

    cap = int(max(z["p1_length"].max(), z["p2_length"].max())) + 3
    jump_cap = int(max(z["p1_jump_locs"].shape[1], z["p2_jump_locs"].shape[1])) + 2
    want_moves = np.full((n, cap), -1, np.int8)
    want_locs = np.full((n, jump_cap, 2), -1, np.int16)
    for i in range(n):
        mv, jl = pick("moves")[i], pick("jump_locs")[i]
        want_moves[i, :len(mv)] = mv
        want_locs[i, :len(jl)] = jl
    fin = np.stack(pick("final"))
    won = np.asarray(pick("won"))
    play = np.stack([won, fin[:, 0], fin[:, 1], fin[:, 2], z["p1_iterations"],
                     np.where(final == 2, z["p2_iterations"], 0)], axis=1).astype(np.int32)
    assert (fin[:, 3] == z["stats"][:, 5]).all()
    want = {"stats": z["stats"], "loss": z["loss"], "won": won != 0, "play": play, "moves": want_moves,
            "length": np.asarray(pick("length"), np.int32), "jump_locs": want_locs}
    with SmbEvaluator(grids.shape[1:], DEV, solver_power=power, max_levels=max_levels or n) as ev:
        assert_same(ev.evaluate(grids, cap=cap, jump_cap=jump_cap), want, "default weights")
        ev.check_errors()
    alt = dict(zip(R.STAT_KEYS, z["alt_weights"].tolist()))
    with SmbEvaluator(grids.shape[1:], DEV, solver_power=power, weights=alt, max_levels=max_levels or n) as ev:
        got = ev.evaluate(grids, playthrough=False)
        assert set(got) == {"stats", "loss", "won", "play"}
        assert np.array_equal(got["loss"].cpu().numpy(), z["loss_alt"]) and np.array_equal(got["stats"].cpu().numpy(), z["stats"])


@pytest.mark.parametrize("power", [10000, 300])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_rules(shape, power):
    maps, answers = levels_and_rules(shape[0], shape[1], power)
    with SmbEvaluator(shape, DEV, solver_power=power, max_levels=64) as ev:
        got = ev.evaluate(torch.from_numpy(maps.copy()).to(DEV), cap=512, jump_cap=64)
        assert_same(got, expect(answers, 512, 64), f"{shape} power {power}")
        ev.check_errors()


def test_batch_sizes_and_successive_launches():
    maps, answers = levels_and_rules(16, 24, 10000)
    big = np.concatenate([maps, maps[:1]])  # 65 levels
    with SmbEvaluator((16, 24), DEV, max_levels=128) as ev:
        assert_same(ev.evaluate(maps[:1]), expect(answers[:1], 512, 64), "n = 1")
        assert_same(ev.evaluate(maps[5]), expect(answers[5:6], 512, 64), "one 2-D map")
        assert_same(ev.evaluate(big), expect(answers + answers[:1], 512, 64), "n = 65")
    with SmbEvaluator((16, 24), DEV, max_levels=16) as ev:  # 65 levels as launches of 16, 16, 16, 16, 1
        assert_same(ev.evaluate(big), expect(answers + answers[:1], 512, 64), "above max_levels")
        ev.check_errors()


def test_same_level_at_different_batch_positions():
    maps, answers = levels_and_rules(16, 116, 10000)
    order = [3, 0, 3, 7, 3, 1, 2, 3]
    with SmbEvaluator((16, 116), DEV, max_levels=8) as ev:
        got = ev.evaluate(maps[order])
    assert_same(got, expect([answers[i] for i in order], 512, 64))
    for k in got:
        rows = got[k].cpu().numpy()[[0, 2, 4, 7]]
        assert all(np.array_equal(rows[0], r) for r in rows[1:]), k


def test_dirty_workspace_does_not_matter():
    hard_maps, hard = levels_and_rules(16, 116, 10000)
    walled = [i for i in range(64) if not hard[i][1]["won"]][:16]  # long searches: they fill the slots
    easy_maps = np.stack([SL.make("structured", 900 + i, 16, 116) for i in range(16)])
    easy = [R.get_stats(m, 10000) for m in easy_maps]
    with SmbEvaluator((16, 116), DEV, max_levels=16) as ev:
        ev._workspace.fill_(-1)
        assert_same(ev.evaluate(hard_maps[walled]), expect([hard[i] for i in walled], 512, 64), "hard")
        assert_same(ev.evaluate(easy_maps), expect(easy, 512, 64), "easy after hard")


def test_caps_truncate_while_counts_stay_full():
    maps, answers = levels_and_rules(16, 116, 10000)
    assert max(len(r["moves"]) for _, r in answers) > 40 and max(r["jumps"] for _, r in answers) > 3
    with SmbEvaluator((16, 116), DEV, max_levels=64) as ev:
        got = ev.evaluate(maps, cap=40, jump_cap=3)
        assert_same(got, expect(answers, 40, 3))
        assert int(got["length"].max()) > 40 and int(got["stats"][:, 5].max()) > 3
        got = ev.evaluate(maps, cap=1, jump_cap=1)
        assert_same(got, expect(answers, 1, 1))


def test_tile_id_above_6_reads_as_empty_and_raises_bit_0():
    maps, _ = levels_and_rules(16, 24, 10000)
    clean = maps[:4].copy()
    dirty = clean.copy()
    dirty[2][(clean[2] == 0) & (np.arange(24)[None, :] % 3 == 0)] = 9
    assert (dirty == 9).any()
    with SmbEvaluator((16, 24), DEV, max_levels=4) as ev:
        want = ev.evaluate(clean)
        ev.check_errors()
        got = ev.evaluate(dirty)
        for k in want:
            assert torch.equal(got[k], want[k]), k
        with pytest.raises(ValueError):
            ev.check_errors()
        ev.check_errors()  # the check clears the bit


def test_evaluate_under_graph_capture():
    maps, answers = levels_and_rules(16, 24, 10000)
    static = torch.from_numpy(maps.copy()).to(DEV)
    with SmbEvaluator((16, 24), DEV, max_levels=64) as ev:
        eager = {k: v.clone() for k, v in ev.evaluate(static).items()}
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            ev.evaluate(static)
        torch.cuda.current_stream(DEV).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = ev.evaluate(static)
        for v in captured.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(captured[k], eager[k]), k
        assert_same(captured, expect(answers, 512, 64))
        ev.check_errors()
