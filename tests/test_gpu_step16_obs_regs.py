"""encode_obs16_regs of step16_kernel (csrc/step16/: six unconditional border stores per lane, the map part of a row built in
registers and written to LDS as dwords) against step_kernel's encoder, byte for byte: the twin engines of
tests/step16_twins.py, compared after EVERY step on observation, reward, done, statistics and the exported state image.  Both
observation buffers are filled with 0xAA before every step, so a chunk that is left out, or written at the wrong wrap, shows.
Run on the GPU box:  python -m pytest tests/test_gpu_step16_obs_regs.py -m gpu
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from step16_twins import EMPTY, _compare, _pair, _same  # noqa: E402

POISON = 0xAA


def _step(new, old, a, t):
    """one poisoned step of both engines, compared; returns the done flags"""
    new._obs.fill_(POISON)
    old._obs.fill_(POISON)
    dev_a = torch.as_tensor(np.asarray(a), dtype=torch.int32).to(new.device)
    on, oo = new.step(dev_a), old.step(dev_a)
    _compare(new, old, on, oo, t)
    return on[2].cpu().numpy()


def _reset(new, old, **kw):
    new._obs.fill_(POISON)
    old._obs.fill_(POISON)
    _same(new.reset(**kw)[0], old.reset(**kw)[0], "reset obs")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 8])
def test_narrow_520_steps_cover_every_scan_position_twice(n):
    """all 256 positions twice: every pos1 % 4 (the alignment shift), pos1 = 0 and 15 (the map's bytes at both ends of the
    row), every pos0 (every wrap point of the border range; 0 and 15: no wrap in the first store, wrap in all but the
    first); partial waves (1, 3, 5 envs), a full one, two"""
    new, old = _pair("narrow", n, 300 + np.arange(n), True)
    _reset(new, old)
    a = torch.randint(0, new.num_actions, (520, n), generator=torch.Generator().manual_seed(100 + n), dtype=torch.int32).numpy()
    seen = set()
    for t in range(520):
        seen.update(map(tuple, new.get_state().pos.cpu().numpy()[:, :2].tolist()))
        _step(new, old, a[t], t)
    assert len(seen) == 256, "every scan position was encoded"
    new.check_errors(); old.check_errors()


def test_uniform_and_striped_maps_kept_through_a_whole_scan():
    """all-empty, all-solid and alternating columns (both parities), two waves: every dword form of the map part and both
    edge dwords differ from the border pattern.  The action re-places the tile under the scan position, so the maps stay."""
    n = 8
    cols = np.tile(np.arange(16) % 2, (16, 1))
    maps = np.stack([np.zeros((16, 16), np.int64), np.ones((16, 16), np.int64), cols, 1 - cols] * 2).astype(np.uint8)
    new, old = _pair("narrow", n, 20 + np.arange(n), True)
    _reset(new, old, init_grids=maps)
    for t in range(260):
        pos = new.get_state().pos.cpu().numpy()[:, :2]
        a = EMPTY["narrow"] + maps[np.arange(n), pos[:, 0], pos[:, 1]].astype(np.int32)
        done = _step(new, old, a, t)
        assert not done.any(), "no reset: the maps are the given ones throughout"
    ref = np.eye(3, dtype=np.uint8)
    pos = new.get_state().pos.cpu().numpy()[:, :2]
    obs = new._obs.cpu().numpy().reshape(n, 32, 32, 3)
    for e in range(n):
        want = ref[np.pad(maps[e].astype(np.int64) + 1, 16)[pos[e, 0]:pos[e, 0] + 32, pos[e, 1]:pos[e, 1] + 32]]
        assert np.array_equal(obs[e], want), f"env {e}: the last observation against the padded window"
    new.check_errors(); old.check_errors()


def _walk(new, old, targets, t0):
    """move every turtle to its target cell (rows first, then columns; an env that has arrived places tiles)"""
    n = len(targets)
    pos = new.get_state().pos.cpu().numpy()[:, :2].copy()
    t = t0
    for _ in range(32):
        a = np.zeros(n, np.int32)
        for e in range(n):
            (r, c), (tr, tc) = pos[e], targets[e]
            if r != tr:
                a[e] = 0 if r > tr else 1
                pos[e, 0] += -1 if r > tr else 1
            elif c != tc:
                a[e] = 2 if c > tc else 3
                pos[e, 1] += -1 if c > tc else 1
            else:
                a[e] = EMPTY["turtle"] + (t + e) % 2
        _step(new, old, a, t)
        t += 1
    assert np.array_equal(new.get_state().pos.cpu().numpy()[:, :2], np.asarray(targets)), "the turtles stand where they were sent"
    return t


def test_turtle_four_envs_of_a_wave_on_rows_0_5_10_15_and_columns_0_1_2_3():
    """the four groups of a wave with four different wrap points (six unconditional trips where the conditional form ran up
    to twelve) and all four alignment shifts at once; then 100 random steps"""
    n = 8
    new, old = _pair("turtle", n, 70 + np.arange(n), True)
    _reset(new, old)
    t = _walk(new, old, [(0, 0), (5, 1), (10, 2), (15, 3), (15, 0), (10, 1), (5, 2), (0, 3)], 0)
    g = torch.Generator().manual_seed(8)
    for k in range(100):
        _step(new, old, torch.randint(0, new.num_actions, (n,), generator=g, dtype=torch.int32).numpy(), t + k)
    new.check_errors(); old.check_errors()


@pytest.mark.parametrize("n,steps", [(5, 260), (344, 40)])
def test_non_temporal_store_flavour(n, steps):
    """PCGRL_OBS_NT_MB=1 (read at pcgrl_create).  At 5 envs a launch writes 15 KB, below the megabyte that sets Params::obs16
    bit 1, so that case runs the switch on the write-through flavour; 344 envs x 3072 bytes >= 1 MB take the non-temporal one."""
    assert "PCGRL_OBS_NT_MB" not in os.environ
    os.environ["PCGRL_OBS_NT_MB"] = "1"
    try:
        new, old = _pair("narrow", n, 7000 + np.arange(n), True, change_percentage=0.02)
    finally:
        del os.environ["PCGRL_OBS_NT_MB"]
    _reset(new, old)
    g = torch.Generator().manual_seed(n)
    for t in range(steps):
        _step(new, old, torch.randint(0, new.num_actions, (n,), generator=g, dtype=torch.int32).numpy(), t)
    new.check_errors(); old.check_errors()


def test_episode_ends_with_auto_reset_inside_the_run():
    """max_changes = 5 (change_percentage 0.02): every env ends episodes within the 520 steps, and the observation of the
    step that resets is the new episode's map and position"""
    n = 5
    new, old = _pair("narrow", n, 900 + np.arange(n), True, change_percentage=0.02)
    _reset(new, old)
    g = torch.Generator().manual_seed(55)
    n_done = np.zeros(n, np.int64)
    for t in range(520):
        n_done += _step(new, old, torch.randint(0, new.num_actions, (n,), generator=g, dtype=torch.int32).numpy(), t)
    assert (n_done >= 1).all(), "every env ended an episode and was reset inside the kernel"
    new.check_errors(); old.check_errors()


@pytest.mark.parametrize("n", [8192, 8196])
def test_both_sides_of_the_batch_size_at_which_the_encoder_changes(n):
    """launches of up to 8 192 envs take encode_obs16_regs, larger ones encode_obs16: the last size of the one and the first
    (a multiple of four, one wave pair more) of the other"""
    new, old = _pair("narrow", n, 1 + np.arange(n), True, change_percentage=0.02)
    _reset(new, old)
    g = torch.Generator().manual_seed(n)
    for t in range(24):
        _step(new, old, torch.randint(0, new.num_actions, (n,), generator=g, dtype=torch.int32).numpy(), t)
    new.check_errors(); old.check_errors()


def _capture(env, static_a):
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for k in range(static_a.shape[0]):
                env._obs.fill_(POISON)
                out = env.step(static_a[k])
    torch.cuda.current_stream().wait_stream(side)
    return graph, out


def test_captured_graph_of_20_steps_replayed_twice():
    n, K = 8, 20
    new, old = _pair("narrow", n, 190 + np.arange(n), True, change_percentage=0.02)
    _reset(new, old)
    g = torch.Generator().manual_seed(6)
    _step(new, old, torch.randint(0, 2, (n,), generator=g, dtype=torch.int32).numpy(), -1)  # (eager warm-up before the capture)
    static_a = torch.zeros((K, n), dtype=torch.int32, device=new.device)
    gn, out_n = _capture(new, static_a)
    go, out_o = _capture(old, static_a)
    for rnd in range(2):
        static_a.copy_(torch.randint(0, 2, (K, n), generator=g, dtype=torch.int32))
        gn.replay(); go.replay()
        torch.cuda.synchronize()
        _compare(new, old, out_n, out_o, f"replay {rnd}")
    new.check_errors(); old.check_errors()
