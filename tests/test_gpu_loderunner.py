"""Lode Runner levels on the device (control_pcgrl_amd.loderunner.LodeRunnerEvaluator, csrc/loderunner/pcgrl_loderunner.h):
the kernel against the fixtures recorded from the reference with its clock stopped (tests/golden/loderunner) and against the
plain-Python rules (tests/loderunner_rules.py) on generated levels (tests/loderunner_levels.py).  Every output is compared bit
for bit, the doubles as their 64-bit patterns."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

from fixture_cases import fixture_cases
import loderunner_levels as LL
import loderunner_rules as R
from control_pcgrl_amd.loderunner import LodeRunnerEvaluator

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loderunner")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))
CASES, CASE_IDS = fixture_cases(FILES)  # each file as ever, and split into several launches
DEV = "cuda:0"
# levels per shape: fewer at 16 x 32, where the plain-Python rules take tens of milliseconds per level
GENERATED = [(8, 12, 2000), (4, 4, 2000), (1, 5, 2000), (5, 7, 2000), (16, 32, 60)]


@functools.lru_cache(maxsize=None)
def levels_and_rules(h, w, n, seed=1):
    """n generated maps of every kind and what the rules say about each; computed once per shape and shared: the tests copy
    before they change a map."""
    maps = LL.mixed(seed, n, h, w)
    return maps, tuple(R.get_stats(m) for m in maps)


def expect(maps, answers, gold_cap, weights=None):
    """The evaluator's outputs, as the rules give them."""
    n = len(maps)
    out = {"stats": np.zeros((n, 5)), "loss": np.zeros(n), "play": np.zeros((n, 4), np.int32), "error": np.zeros(n, np.int32)}
    if gold_cap:
        out["gold_state"] = np.full((n, gold_cap), -1, np.int8)
        out["gold_dist"] = np.zeros((n, gold_cap), np.int16)
    for i, (stats, rec) in enumerate(answers):
        out["stats"][i] = stats
        out["loss"][i] = R.loss(stats, weights)
        golds = int(stats[2])
        k = min(gold_cap, golds)
        if rec is None:
            out["play"][i] = [0, -1, -1, 0]
            if gold_cap:
                out["gold_state"][i, :k] = 0
        else:
            out["play"][i] = [1, rec["landing"][0], rec["landing"][1], rec["collected"]]
            if gold_cap:
                out["gold_state"][i, :k] = rec["state"][:k]
                out["gold_dist"][i, :k] = rec["dist"][:k]
    out["win"], out["path_length"] = out["stats"][:, 3], out["stats"][:, 4]
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same(got, want, what=""):
    assert set(got) == set(want), (set(got), set(want))
    for k in want:
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape)
        bad = np.nonzero((bits(g) != bits(want[k])).reshape(len(g), -1).any(axis=1))[0]
        assert bad.size == 0, (what, k, "levels", bad[:8].tolist(), g[bad[0]].tolist(), want[k][bad[0]].tolist())


@pytest.mark.parametrize("path,max_levels", CASES, ids=CASE_IDS)
def test_kernel_equals_fixtures(path, max_levels):
    z = np.load(path)
    grids = z["grids"]
    n, cap = len(grids), z["gold_state"].shape[1]
    want = {"stats": z["stats"], "loss": np.array([R.loss(s) for s in z["stats"]]), "error": np.zeros(n, np.int32),
            "play": np.column_stack([z["stats"][:, 0] == 1, z["landing"], z["collected"]]).astype(np.int32),
            "gold_state": z["gold_state"], "gold_dist": z["gold_dist"], "win": z["stats"][:, 3], "path_length": z["stats"][:, 4]}
    with LodeRunnerEvaluator(grids.shape[1:], DEV, **({"max_levels": max_levels} if max_levels else {})) as ev:
        assert_same(ev.evaluate(grids, gold_cap=cap), want, os.path.basename(path))
        ev.check_errors()


@pytest.mark.parametrize("h,w,n", GENERATED, ids=[f"{h}x{w}" for h, w, _ in GENERATED])
def test_kernel_equals_rules_on_generated_levels(h, w, n):
    maps, answers = levels_and_rules(h, w, n)
    cap = max(1, max(int(s[2]) for s, _ in answers))
    with LodeRunnerEvaluator((h, w), DEV) as ev:
        assert_same(ev.evaluate(maps, gold_cap=cap), expect(maps, answers, cap), f"{h}x{w}")
        ev.check_errors()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(n):
    maps, answers = levels_and_rules(8, 12, 2000)
    with LodeRunnerEvaluator((8, 12), DEV) as ev:
        assert_same(ev.evaluate(maps[:n]), expect(maps[:n], answers[:n], 32), f"n={n}")


def test_batches_above_max_levels_run_as_successive_launches():
    maps, answers = levels_and_rules(8, 12, 2000)
    with LodeRunnerEvaluator((8, 12), DEV, max_levels=3) as ev:
        assert_same(ev.evaluate(maps[:8]), expect(maps[:8], answers[:8], 32))


@pytest.mark.parametrize("h,w,n", [(4, 4, 4500), (16, 32, 900)], ids=["4x4", "16x32"])
def test_more_levels_than_blocks(h, w, n):
    """above 4096 levels (839 at 16 x 32, where the workspace stops at 640 MiB) a block strides over several levels on one
    workspace slot; the 16 x 32 maps are the 60 of the test above, repeated"""
    maps, answers = levels_and_rules(h, w, n) if (h, w) == (4, 4) else levels_and_rules(16, 32, 60)
    reps = -(-n // len(maps))
    maps, answers = np.concatenate([maps] * reps)[:n], (answers * reps)[:n]
    with LodeRunnerEvaluator((h, w), DEV, max_levels=n) as ev:
        assert_same(ev.evaluate(maps, gold_cap=4), expect(maps, answers, 4))


def test_gold_cap_below_the_gold_count_and_zero():
    maps = LL.batch("gold", 5, 32, 8, 12)
    answers = tuple(R.get_stats(m) for m in maps)
    assert min(int(s[2]) for s, _ in answers) > 3 and max(int(s[2]) for s, _ in answers) > 32  # more than one round of searches
    with LodeRunnerEvaluator((8, 12), DEV) as ev:
        full = ev.evaluate(maps, gold_cap=48)
        assert_same(full, expect(maps, answers, 48))
        cut = ev.evaluate(maps, gold_cap=3)
        assert_same(cut, expect(maps, answers, 3))
        assert torch.equal(cut["stats"], full["stats"]) and torch.equal(cut["play"], full["play"])  # the totals stay complete
        none = ev.evaluate(maps, gold_cap=0)
        assert "gold_state" not in none and "gold_dist" not in none
        assert_same(none, expect(maps, answers, 0))


def test_every_optional_output_null():
    import ctypes as C
    from control_pcgrl_amd import _lib
    from control_pcgrl_amd.loderunner import loderunner_config
    maps, answers = levels_and_rules(8, 12, 2000)
    n = 70
    L = _lib.lib()
    g = torch.from_numpy(maps[:n].copy()).to(DEV)
    nbytes = L.pcgrl_loderunner_workspace_bytes(n, 8, 12)
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=DEV)
    stats = torch.empty((n, 5), dtype=torch.float64, device=DEV)
    cfg = loderunner_config((8, 12))
    _lib.check(L.pcgrl_loderunner_evaluate(C.byref(cfg), n, g.data_ptr(), ws.data_ptr(), nbytes, 32, stats.data_ptr(), None, None,
                                           None, None, None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert_same({"stats": stats}, {"stats": expect(maps[:n], answers[:n], 0)["stats"]})


def test_dirty_workspace_and_weights():
    maps, answers = levels_and_rules(8, 12, 2000)
    w = {"player": 3, "enemies": 0.5, "gold": 2, "win": 7, "path-length": 0.25}
    with LodeRunnerEvaluator((8, 12), DEV, weights=w) as ev:
        first = {k: v.clone() for k, v in ev.evaluate(maps[:256]).items()}
        ev._workspace.fill_(-1)
        second = ev.evaluate(maps[:256])
        for k in first:
            assert torch.equal(first[k], second[k]), k
        assert_same(second, expect(maps[:256], answers[:256], 32, w))


def test_tile_id_above_7_sets_the_error_bit():
    maps, answers = levels_and_rules(8, 12, 2000)
    dirty = maps[:16].copy()
    dirty[5, 3, 4] = 9
    clean = dirty.copy()
    clean[5, 3, 4] = 0  # read as empty
    want = expect(clean, tuple(R.get_stats(m) for m in clean), 32)
    want["error"][5] = 1
    with LodeRunnerEvaluator((8, 12), DEV) as ev:
        assert_same(ev.evaluate(dirty), want)  # the rest of the batch is unaffected
        with pytest.raises(ValueError):
            ev.check_errors()
        ev.check_errors()  # cleared


def test_evaluate_under_graph_capture():
    maps, answers = levels_and_rules(8, 12, 2000)
    static = torch.from_numpy(maps[:96].copy()).to(DEV)
    with LodeRunnerEvaluator((8, 12), DEV, max_levels=64) as ev:
        eager = {k: v.clone() for k, v in ev.evaluate(static).items()}
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            ev.evaluate(static)
        torch.cuda.current_stream(DEV).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = ev.evaluate(static)
        for k in ("stats", "loss", "play", "gold_state", "gold_dist", "error"):
            captured[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(captured[k], eager[k]), k
        assert_same(captured, expect(maps[:96], answers[:96], 32))
        ev.check_errors()


def test_two_evaluators_on_two_streams():
    maps, answers = levels_and_rules(8, 12, 2000)
    a_maps, b_maps = torch.from_numpy(maps[:512].copy()).to(DEV), torch.from_numpy(maps[512:1024].copy()).to(DEV)
    with LodeRunnerEvaluator((8, 12), DEV) as ea, LodeRunnerEvaluator((8, 12), DEV) as eb:
        serial = (ea.evaluate(a_maps), eb.evaluate(b_maps))
        torch.cuda.synchronize()
        sa, sb = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
        with torch.cuda.stream(sa):
            ra = ea.evaluate(a_maps)
        with torch.cuda.stream(sb):
            rb = eb.evaluate(b_maps)
        torch.cuda.synchronize()
        for got, want in zip((ra, rb), serial):
            for k in want:
                assert torch.equal(got[k], want[k]), k
        assert_same(ra, expect(maps[:512], answers[:512], 32))
        assert_same(rb, expect(maps[512:1024], answers[512:1024], 32))
