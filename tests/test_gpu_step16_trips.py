"""The trip control and the wrap-up of step16_kernel's sweeps (csrc/step16/): the trip body is laid out twice, so whether a
group dies in an odd or an even trip, and whether the wave's last trip is one, matters; length, last level and far cell come
out of one max-reduction of keys.  As in tests/test_gpu_step16.py a PCGRL_STEP16=0 engine (step_kernel) is stepped next to a
default one and everything -- observation, reward, done, statistics, the exported state image -- is compared after every
step, statistics, reward and done also against the CPU oracle; the cached planes are held to tests/step_masks_numpy.py.
Run on the GPU box:  python -m pytest tests/test_gpu_step16_trips.py -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import pcgrl_oracle as po  # noqa: E402  (checker only)
from step16_twins import EMPTY, REW_TOL, SHAPE, _compare, _pair, _same, _step_all  # noqa: E402
from step_masks_numpy import check_all  # noqa: E402
from test_gpu_step16 import _capture, _snake, _solid  # noqa: E402

REPS = ["narrow", "turtle"]


def _corridor(L):
    """the first L cells of the serpentine open; opening cell L makes a path of L levels from either end"""
    g = _solid()
    for (r, c) in _snake()[:L]:
        g[r, c] = 0
    return g


def _star(arms, hook=0):
    """arms (up, down, left, right) around the open centre (8, 8); `hook` more cells along row 0 at the top of a full up arm"""
    g = _solid()
    g[8, 8] = 0
    for (dr, dc), k in zip(((-1, 0), (1, 0), (0, -1), (0, 1)), arms):
        for i in range(1, k + 1):
            g[8 + dr * i, 8 + dc * i] = 0
    if hook:
        assert arms[0] == 8
        g[0, 9:9 + hook] = 0
    return g


def _run(rep, cases, more_steps=8):
    """cases: (map, cell of the first edit, tile it gets: 0 empty / 1 solid).  Returns statistics before and after that edit."""
    n = len(cases)
    grids = np.stack([c[0] for c in cases])
    pos = np.array([c[1] for c in cases], np.int32)
    first = np.array([EMPTY[rep] + c[2] for c in cases], np.int32)
    seeds = 4100 + np.arange(n)
    new, old = _pair(rep, n, seeds, False)
    orc = po.OracleVecEnv("binary", rep, SHAPE, n, seeds=seeds, threads=4)
    o_n, _ = new.reset(init_grids=torch.as_tensor(grids), init_pos=torch.as_tensor(pos))
    o_o, _ = old.reset(init_grids=torch.as_tensor(grids), init_pos=torch.as_tensor(pos))
    _same(o_n, o_o, "reset obs")
    orc.reset(init_grids=grids, init_pos=pos)
    before = new.get_state().stats.cpu().numpy().copy()
    assert np.array_equal(before, orc.get_state()["stats"])
    _step_all(new, old, orc, first, 0, False)
    check_all(new)
    check_all(old)
    after = new.get_state().stats.cpu().numpy().copy()
    g = torch.Generator().manual_seed(11)
    for t in range(1, 1 + more_steps):
        a = torch.randint(0, new.num_actions, (n,), generator=g, dtype=torch.int32).numpy()
        _step_all(new, old, orc, a, t, False)
        check_all(new)
    new.check_errors(); old.check_errors()
    return before, after


@pytest.mark.parametrize("rep", REPS)
def test_corridors_ending_in_every_residue_mod_12(rep):
    """lengths 1..40: both sweeps of a corridor of L levels die in trip L // 6 + 1 on level L % 6 of it.  First ten waves:
    four consecutive lengths each (the groups of a wave die on different levels, some in different trips, and the wave's last
    trip is odd or even); then every length four times (a wave whose four groups die in the same trip on the same level, and
    a wave that leaves the loop after every number of trips from 1 to 7)."""
    snake = _snake()
    lengths = list(range(1, 41)) + [L for L in range(1, 41) for _ in range(4)]
    assert {L % 12 for L in lengths[:40]} == set(range(12))
    _, after = _run(rep, [(_corridor(L), snake[L], 0) for L in lengths], more_steps=4)
    for i, L in enumerate(lengths):
        assert tuple(after[i]) == (1, L), (i, L, after[i])


@pytest.mark.parametrize("rep", REPS)
def test_groups_that_die_in_different_trips_and_groups_without_a_seed(rep):
    snake = _snake()
    iso = _solid(); iso[2, 3] = 0
    cases = []
    # a wave whose four groups die in trips 1, 2, 3 and 4 -- in this order, in the reverse, and mixed
    for order in ((3, 9, 15, 21), (21, 15, 9, 3), (15, 3, 21, 9)):
        cases += [(_corridor(L), snake[L], 0) for L in order]
    # groups without a seed in the first sweeps (an edit that changes nothing; an isolated cell that appears on an all-solid
    # map and one that disappears: nothing but isolated cells to sweep from) next to a group that runs ten trips
    cases += [(_corridor(30), snake[5], 0), (_corridor(57), snake[57], 0), (_solid(), (9, 9), 0), (iso, (2, 3), 1)]
    # ... and a wave in which only the last group has anything to sweep, for eleven trips
    cases += [(_solid(), (0, 0), 1), (_solid(), (15, 15), 1), (_corridor(12), snake[3], 0), (_corridor(63), snake[63], 0)]
    before, after = _run(rep, cases)
    for i, L in enumerate((3, 9, 15, 21, 21, 15, 9, 3, 15, 3, 21, 9)):
        assert tuple(after[i]) == (1, L)
    assert np.array_equal(before[12], after[12]) and tuple(after[13]) == (1, 57)
    assert tuple(after[14]) == (1, 0) and tuple(after[15]) == (0, 0)
    assert np.array_equal(before[18], after[18]) and tuple(after[19]) == (1, 63)


@pytest.mark.parametrize("rep", REPS)
def test_splits_into_small_pieces_beside_a_long_one_and_a_merge_of_four(rep):
    """the centre of a star closes: 2, 3 and 4 pieces, those of 1..5 cells beside a long one that comes first (up, with a
    hook along row 0: 15 cells) or last (down) in row-major order of the pieces' first cells; the centre opens: four
    components become one"""
    splits = [((8, 1, 0, 0), 7), ((1, 7, 0, 0), 0), ((8, 0, 0, 3), 7), ((0, 7, 2, 0), 0),            # 2 pieces
              ((8, 2, 5, 0), 7), ((2, 7, 0, 4), 0), ((8, 0, 1, 1), 7), ((1, 7, 5, 0), 0),            # 3 pieces
              ((8, 1, 3, 5), 7), ((1, 7, 4, 2), 0), ((8, 5, 1, 3), 7), ((4, 7, 2, 1), 0), ((5, 7, 5, 5), 0)]  # 4 pieces
    cases = []
    for arms, hook in splits:
        cases.append((_star(arms, hook), (8, 8), 1))
    merges = [(8, 1, 3, 5), (1, 7, 4, 2), (2, 7, 4, 6), (1, 3, 1, 5)]
    for arms in merges:
        g = _star(arms, 7 if arms[0] == 8 else 0)
        g[8, 8] = 1
        cases.append((g, (8, 8), 0))
    before, after = _run(rep, cases)
    for i, (arms, hook) in enumerate(splits):
        pieces = sum(1 for k in arms if k > 0)
        longest = max(k + (hook if j == 0 else 0) for j, k in enumerate(arms)) - 1
        assert before[i][0] == 1 and tuple(after[i]) == (pieces, longest), (arms, before[i], after[i])
    for i, arms in enumerate(merges, start=len(splits)):
        assert before[i][0] == 4 and after[i][0] == 1, (arms, before[i], after[i])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 8])
@pytest.mark.parametrize("rep", REPS)
def test_small_batches_across_an_auto_reset(rep, n):
    """a partial wave (1, 3 envs), one full wave, a wave and one env, one full workgroup; max_changes = 5 ends an episode of
    every env within the run"""
    seeds = 7300 + np.arange(n)
    kw = dict(change_percentage=0.02)
    new, old = _pair(rep, n, seeds, True, **kw)
    orc = po.OracleVecEnv("binary", rep, SHAPE, n, seeds=seeds, threads=4, **kw)
    _same(new.reset()[0], old.reset()[0], "reset obs")
    orc.reset()
    g = torch.Generator().manual_seed(100 + n)
    n_done = 0
    for t in range(60):
        a = torch.randint(0, new.num_actions, (n,), generator=g, dtype=torch.int32).numpy()
        n_done += int(_step_all(new, old, orc, a, t, True).sum())
        check_all(new)
    assert n_done >= n, "every env ended an episode"
    new.check_errors(); old.check_errors()


def test_captured_graph_of_20_steps_on_corridors():
    """20 captured launches on maps whose sweeps take many trips (corridors of 20..45 cells, the scan edits along them)"""
    n, K = 13, 20
    seeds = 520 + np.arange(n)
    grids = np.stack([_corridor(20 + 2 * i) for i in range(n)])
    pos = np.zeros((n, 2), np.int32)
    new, old = _pair("narrow", n, seeds, False)
    orc = po.OracleVecEnv("binary", "narrow", SHAPE, n, seeds=seeds, threads=4)
    for env in (new, old):
        env.reset(init_grids=torch.as_tensor(grids), init_pos=torch.as_tensor(pos))
    orc.reset(init_grids=grids, init_pos=pos)
    g = torch.Generator().manual_seed(3)
    a0 = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32)
    _step_all(new, old, orc, a0.numpy(), -1, False)  # (eager warm-up before the capture)
    static_a = torch.zeros((K, n), dtype=torch.int32, device=new.device)
    gn, out_n = _capture(new, static_a)
    go, out_o = _capture(old, static_a)
    for rnd in range(2):
        a = torch.randint(0, 2, (K, n), generator=g, dtype=torch.int32)
        static_a.copy_(a)
        gn.replay(); go.replay()
        torch.cuda.synchronize()
        _compare(new, old, out_n, out_o, f"replay {rnd}")
        for k in range(K):
            _, orew, odone, ostats = orc.step(a[k].numpy(), auto_reset=False, want_obs=False)
        assert np.array_equal(out_n[4]["stats"].cpu().numpy(), ostats), f"stats vs oracle, replay {rnd}"
        assert np.max(np.abs(out_n[1].cpu().numpy().astype(np.float64) - orew)) <= REW_TOL
        assert np.array_equal(out_n[2].cpu().numpy(), odone)
        check_all(new)
    new.check_errors(); old.check_errors()
