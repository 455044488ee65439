"""step16_kernel (csrc/step16/) against step_kernel, bit for bit: two engines from the same seeds and actions, one created
with PCGRL_STEP16=0 (the development switch that keeps the binary 16x16 step on step_kernel), compared after EVERY step on
observation, reward, done, statistics and the exported state image (pcgrl_export_state: planes with the fars / best masks
and the PREFLOOD plane, records, RNG streams); statistics, reward and done also against the CPU oracle.
Run on the GPU box:  python -m pytest tests/test_gpu_step16.py -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import pcgrl_oracle as po  # noqa: E402  (checker only)
from step16_twins import EMPTY, REW_TOL, SHAPE, _compare, _pair, _same, _step_all  # noqa: E402,F401


@pytest.mark.parametrize("n", [1, 3, 8, 13, 64])
@pytest.mark.parametrize("rep", ["narrow", "turtle"])
def test_random_steps_across_an_auto_reset(rep, n):
    """partial waves (1, 3 envs), a partial workgroup (13 = three waves and one env), full ones; max_changes = 5 (2 % of
    256 cells) ends every episode within the run, so the in-kernel reset, its RNG replay in the observe wave and the
    episode latch are crossed"""
    seeds = 900 + np.arange(n)
    kw = dict(change_percentage=0.02)
    new, old = _pair(rep, n, seeds, True, **kw)
    orc = po.OracleVecEnv("binary", rep, SHAPE, n, seeds=seeds, threads=4, **kw)
    _same(new.reset()[0], old.reset()[0], "reset obs")
    orc.reset()
    g = torch.Generator().manual_seed(n)
    n_done = 0
    for t in range(70):
        a = torch.randint(0, new.num_actions, (n,), generator=g, dtype=torch.int32).numpy()
        n_done += int(_step_all(new, old, orc, a, t, True).sum())
    assert n_done >= n, "every env ended an episode"
    le_n, le_o = new.last_episode(), old.last_episode()
    for f in ("n_episodes", "final_stats", "ep_len", "ep_return"):
        _same(getattr(le_n, f), getattr(le_o, f), f)
    new.check_errors(); old.check_errors()


# ------------------------------------------------------------------------------------------------ injected maps
def _snake():
    """the cells of a serpentine corridor through the map: even rows end to end, joined at alternating ends"""
    cells = []
    for k, r in enumerate(range(0, 16, 2)):
        xs = range(16) if k % 2 == 0 else range(15, -1, -1)
        cells += [(r, x) for x in xs]
        if r + 1 < 16:
            cells.append((r + 1, 15 if k % 2 == 0 else 0))
    return cells


def _solid():
    return np.ones(SHAPE, np.uint8)


def _corner_cases():
    """(name, map, cell of the first edit, tile it gets): 0 = empty (passable), 1 = solid"""
    snake, cases = _snake(), []

    def corridor(L):  # L cells open, the edit opens cell L: a path of L levels from either end
        g = _solid()
        for (r, c) in snake[:L]:
            g[r, c] = 0
        return g

    # four envs of one wave whose sweeps end in different trips (first in the batch: envs 0..3 share a wavefront)
    for L in (3, 9, 15, 40):
        cases.append((f"wave-mix-{L}", corridor(L), snake[L], 0))
    # the last live trip ends on every level of a trip: lengths 0..5 mod 6, short and long
    for L in list(range(13, 19)) + list(range(61, 67)):
        cases.append((f"corridor-{L}", corridor(L), snake[L], 0))
    # ... and the same corridors cut near the middle (two pieces of different length, the sweeps of the peel loop)
    for L in (14, 17, 63):
        cases.append((f"corridor-cut-{L}", corridor(L + 1), snake[L // 2 - 1], 1))

    def star(arms):  # arms (up, down, left, right) of the given lengths around (8, 8)
        g = _solid()
        for (dr, dc), k in zip(((-1, 0), (1, 0), (0, -1), (0, 1)), arms):
            for i in range(1, k + 1):
                g[8 + dr * i, 8 + dc * i] = 0
        return g

    for name, arms in (("2", (3, 5, 0, 0)), ("3", (2, 7, 4, 0)), ("4", (2, 7, 4, 6)), ("4-iso", (1, 3, 1, 5))):
        g = star(arms)
        cases.append((f"merge-{name}", g.copy(), (8, 8), 0))  # the centre opens: the arms become one component
        g[8, 8] = 0
        cases.append((f"split-{name}", g, (8, 8), 1))         # the centre closes: the component falls apart
    # isolated cells: one appears, one disappears, one appears next to nothing on an all-solid map
    g = _solid(); g[2, 3] = 0
    cases.append(("iso-appears", g.copy(), (11, 12), 0))
    cases.append(("iso-disappears", g.copy(), (2, 3), 1))
    cases.append(("iso-first", _solid(), (15, 15), 0))
    # on and off the `best` component: a long corridor (best) and a short one
    g = corridor(30)
    for c in range(4, 9):
        g[14, c] = 0
    cases.append(("off-best-grow", g.copy(), (14, 9), 0))
    cases.append(("off-best-cut", g.copy(), (14, 6), 1))
    cases.append(("on-best-grow", g.copy(), snake[30], 0))
    cases.append(("on-best-cut", g.copy(), snake[11], 1))
    cases.append(("on-best-shrink-below-other", g.copy(), snake[2], 1))
    # the edited cell becomes the component's first cell in row-major order (to the left of it / above it)
    g = _solid(); g[5:9, 5:11] = 0; g[7, 6:9] = 1
    cases.append(("first-cell-left", g.copy(), (5, 4), 0))
    cases.append(("first-cell-above", g.copy(), (4, 9), 0))
    cases.append(("first-cell-removed", g.copy(), (5, 5), 1))
    # an edit that changes nothing (the cell already has the tile)
    cases.append(("no-change", g.copy(), (6, 6), 0))
    return cases


@pytest.mark.parametrize("rep", ["narrow", "turtle"])
def test_injected_maps_hit_the_sweep_corners(rep):
    cases = _corner_cases()
    n = len(cases)
    assert n > 8 and n % 4 != 0  # (several workgroups, the last wave partial)
    grids = np.stack([c[1] for c in cases])
    pos = np.array([c[2] for c in cases], np.int32)
    first = np.array([EMPTY[rep] + c[3] for c in cases], np.int32)
    seeds = 300 + np.arange(n)
    new, old = _pair(rep, n, seeds, False)
    orc = po.OracleVecEnv("binary", rep, SHAPE, n, seeds=seeds, threads=4)
    o_n, _ = new.reset(init_grids=torch.as_tensor(grids), init_pos=torch.as_tensor(pos))
    o_o, _ = old.reset(init_grids=torch.as_tensor(grids), init_pos=torch.as_tensor(pos))
    _same(o_n, o_o, "reset obs")
    orc.reset(init_grids=grids, init_pos=pos)
    before = new.get_state().stats.cpu().numpy().copy()
    assert np.array_equal(before, orc.get_state()["stats"])
    _step_all(new, old, orc, first, 0, False)
    after = new.get_state().stats.cpu().numpy()
    names = [c[0] for c in cases]
    by = {k: (before[i], after[i]) for i, k in enumerate(names)}
    for L in list(range(13, 19)) + list(range(61, 67)):
        assert tuple(by[f"corridor-{L}"][1]) == (1, L), (L, by[f"corridor-{L}"])
    assert by["split-4"][1][0] == 4 and by["split-3"][1][0] == 3 and by["split-2"][1][0] == 2 and by["split-4-iso"][1][0] == 4
    assert by["merge-4"][0][0] == 4 and by["merge-3"][0][0] == 3 and by["merge-2"][0][0] == 2
    assert all(by[f"merge-{k}"][1][0] == 1 for k in ("2", "3", "4", "4-iso"))
    assert by["iso-appears"][1][0] == 2 and by["iso-disappears"][1][0] == 0 and tuple(by["iso-first"][1]) == (1, 0)
    assert np.array_equal(by["no-change"][0], by["no-change"][1])
    # a few more steps from there: the next edits land next to the first one (turtle) or at the scan's start (narrow)
    g = torch.Generator().manual_seed(7)
    for t in range(1, 13):
        a = torch.randint(0, new.num_actions, (n,), generator=g, dtype=torch.int32).numpy()
        _step_all(new, old, orc, a, t, False)
    new.check_errors(); old.check_errors()


def _capture(env, static_a):
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for k in range(static_a.shape[0]):
                out = env.step(static_a[k])
    torch.cuda.current_stream().wait_stream(side)
    return graph, out


def test_captured_graph_of_20_steps():
    n, K = 13, 20
    seeds = 70 + np.arange(n)
    kw = dict(change_percentage=0.02)
    new, old = _pair("narrow", n, seeds, True, **kw)
    orc = po.OracleVecEnv("binary", "narrow", SHAPE, n, seeds=seeds, threads=4, **kw)
    new.reset(); old.reset(); orc.reset()
    g = torch.Generator().manual_seed(2)
    a0 = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32)
    _step_all(new, old, orc, a0.numpy(), -1, True)  # (eager warm-up before the capture)
    static_a = torch.zeros((K, n), dtype=torch.int32, device=new.device)
    gn, out_n = _capture(new, static_a)
    go, out_o = _capture(old, static_a)
    for rnd in range(3):  # 60 steps: every env crosses an auto-reset inside a replay
        a = torch.randint(0, 2, (K, n), generator=g, dtype=torch.int32)
        static_a.copy_(a)
        gn.replay(); go.replay()
        torch.cuda.synchronize()
        _compare(new, old, out_n, out_o, f"replay {rnd}")
        for k in range(K):
            _, orew, odone, ostats = orc.step(a[k].numpy(), auto_reset=True, want_obs=False)
        assert np.array_equal(out_n[4]["stats"].cpu().numpy(), ostats), f"stats vs oracle, replay {rnd}"
        assert np.max(np.abs(out_n[1].cpu().numpy().astype(np.float64) - orew)) <= REW_TOL
        assert np.array_equal(out_n[2].cpu().numpy(), odone)
    assert int(new.last_episode().n_episodes.min()) >= 1
    new.check_errors(); old.check_errors()


def test_update_then_replayed_graph_raises_estale():
    """the captured launch is step16_kernel, which -- like the compile-time step_kernel -- has no code for the statistics
    pcgrl_update leaves stale: a replay after an update reports PCGRL_ESTALE; eager steps take the general kernel"""
    n = 8
    new, old = _pair("narrow", n, 5 + np.arange(n), False)
    new.reset(); old.reset()
    static_a = torch.zeros((1, n), dtype=torch.int32, device=new.device)
    new.step(static_a[0])  # (eager warm-up before the capture)
    old.step(static_a[0])
    gn, _ = _capture(new, static_a)
    g = torch.Generator().manual_seed(4)
    for _ in range(4):
        a = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32).to(new.device)
        new.update(a, want_obs=False); old.update(a, want_obs=False)
    new.check_errors()
    for _ in range(20):
        static_a.copy_(torch.randint(0, 2, (1, n), generator=g, dtype=torch.int32))
        gn.replay()
    with pytest.raises(RuntimeError, match="ESTALE"):
        new.check_errors()
    # eager stepping after an update is the general kernel on both engines: the same results, no error
    new.reset(); old.reset()
    for _ in range(3):
        a = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32).to(new.device)
        new.update(a, want_obs=False); old.update(a, want_obs=False)
    for t in range(6):
        a = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32).to(new.device)
        _compare(new, old, new.step(a), old.step(a), t)
    new.check_errors(); old.check_errors()
