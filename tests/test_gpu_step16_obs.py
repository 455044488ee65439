"""The observation encoder of step16_kernel (encode_obs16, csrc/step16/: border rows from registers first, map rows through
LDS behind them) against step_kernel's, byte for byte: the twin engines of tests/step16_twins.py, compared after EVERY step
on observation, reward, done, statistics and the exported state image.  The observation buffers are filled with 0xAA before
every step, so a chunk the encoder leaves out shows, and so does one it writes twice with different bytes in between.
Run on the GPU box:  python -m pytest tests/test_gpu_step16_obs.py -m gpu
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import pcgrl_oracle as po  # noqa: E402  (checker only)
from step16_twins import EMPTY, REW_TOL, SHAPE, _compare, _pair, _same, _step_all  # noqa: E402,F401

POISON = 0xAA


def _poison(*envs):
    for env in envs:
        env._obs.fill_(POISON)


def _poisoned_step(new, old, orc, a, t, auto_reset=True):
    _poison(new, old)
    return _step_all(new, old, orc, a, t, auto_reset)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 8])
def test_narrow_800_steps_cover_every_scan_position_and_an_episode_end(n):
    """the scan visits all 256 cells three times (pos0 = 0..15: every border / map split of both phases); partial waves
    (1, 3, 5 envs), a full one, two; the episode ends by max_iterations at step 770: the in-kernel reset's pos and map"""
    seeds = 40 + np.arange(n)
    new, old = _pair("narrow", n, seeds, True)
    orc = po.OracleVecEnv("binary", "narrow", SHAPE, n, seeds=seeds, threads=2)
    _poison(new, old)
    _same(new.reset()[0], old.reset()[0], "reset obs")
    orc.reset()
    a = torch.randint(0, new.num_actions, (800, n), generator=torch.Generator().manual_seed(n), dtype=torch.int32).numpy()
    n_done = 0
    for t in range(800):
        n_done += int(_poisoned_step(new, old, orc, a[t], t).sum())
    assert n_done == n, "every env ended its episode once"
    new.check_errors(); old.check_errors()


def _walk(new, old, orc, targets, t0):
    """move every turtle to its target cell (rows first, then columns; an env that has arrived places tiles), then stand
    there for four steps"""
    n = len(targets)
    pos = new.get_state().pos.cpu().numpy()[:, :2].copy()
    t = t0
    for _ in range(34):
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
        _poisoned_step(new, old, orc, a, t)
        t += 1
    assert np.array_equal(new.get_state().pos.cpu().numpy()[:, :2], np.asarray(targets)), "the turtles stand where they were sent"
    return t


def test_turtle_8_envs_in_rows_and_columns_0_15_7_8_of_one_wave():
    """the four groups of a wave at pos0 = 0, 15, 7, 8: every phase-1 trip has a different mask in each group (all map rows
    last, first, and the two middle splits), and the columns 0, 15, 7, 8 put the map's bytes at both ends of an LDS row"""
    n = 8
    seeds = 11 + np.arange(n)
    new, old = _pair("turtle", n, seeds, True)
    orc = po.OracleVecEnv("binary", "turtle", SHAPE, n, seeds=seeds, threads=2)
    _poison(new, old)
    _same(new.reset()[0], old.reset()[0], "reset obs")
    orc.reset()
    t = _walk(new, old, orc, [(0, 0), (15, 15), (7, 7), (8, 8), (0, 15), (15, 0), (7, 8), (8, 7)], 0)
    t = _walk(new, old, orc, [(15, 7), (0, 8), (8, 0), (7, 15), (8, 15), (7, 0), (15, 8), (0, 7)], t)
    g = torch.Generator().manual_seed(3)
    for k in range(200):
        a = torch.randint(0, new.num_actions, (n,), generator=g, dtype=torch.int32).numpy()
        _poisoned_step(new, old, orc, a, t + k)
    new.check_errors(); old.check_errors()


def test_turtle_64_envs_random():
    n = 64
    seeds = 500 + np.arange(n)
    new, old = _pair("turtle", n, seeds, True)
    orc = po.OracleVecEnv("binary", "turtle", SHAPE, n, seeds=seeds, threads=4)
    _poison(new, old)
    _same(new.reset()[0], old.reset()[0], "reset obs")
    orc.reset()
    g = torch.Generator().manual_seed(64)
    for t in range(300):
        a = torch.randint(0, new.num_actions, (n,), generator=g, dtype=torch.int32).numpy()
        _poisoned_step(new, old, orc, a, t)
    rows = new.get_state().pos.cpu().numpy()[:, 0]
    assert len(set(rows.tolist())) >= 8, "the envs of a wave stand in different rows"
    new.check_errors(); old.check_errors()


def test_non_temporal_store_flavour():
    """PCGRL_OBS_NT_MB=1 (read at pcgrl_create): 344 envs x 3072 bytes >= 1 MB per launch sets Params::obs16 bit 1"""
    n = 344
    assert n * 32 * 32 * 3 >= 1_000_000 and n % 4 == 0 and (n // 4) % 2 == 0
    seeds = 7000 + np.arange(n)
    assert "PCGRL_OBS_NT_MB" not in os.environ
    os.environ["PCGRL_OBS_NT_MB"] = "1"
    try:
        new, old = _pair("narrow", n, seeds, True, change_percentage=0.02)
    finally:
        del os.environ["PCGRL_OBS_NT_MB"]
    orc = po.OracleVecEnv("binary", "narrow", SHAPE, n, seeds=seeds, threads=4, change_percentage=0.02)
    _poison(new, old)
    _same(new.reset()[0], old.reset()[0], "reset obs")
    orc.reset()
    g = torch.Generator().manual_seed(344)
    n_done = 0
    for t in range(50):
        a = torch.randint(0, new.num_actions, (n,), generator=g, dtype=torch.int32).numpy()
        n_done += int(_poisoned_step(new, old, orc, a, t).sum())
    assert n_done > 0
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
    seeds = 90 + np.arange(n)
    kw = dict(change_percentage=0.02)
    new, old = _pair("narrow", n, seeds, True, **kw)
    orc = po.OracleVecEnv("binary", "narrow", SHAPE, n, seeds=seeds, threads=2, **kw)
    new.reset(); old.reset(); orc.reset()
    g = torch.Generator().manual_seed(5)
    a0 = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32)
    _poisoned_step(new, old, orc, a0.numpy(), -1)  # (eager warm-up before the capture)
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
            oobs, orew, odone, ostats = orc.step(a[k].numpy(), auto_reset=True)
        assert np.array_equal(out_n[0].cpu().numpy().reshape(n, -1), oobs.reshape(n, -1)), f"obs vs oracle, replay {rnd}"
        assert np.array_equal(out_n[4]["stats"].cpu().numpy(), ostats), f"stats vs oracle, replay {rnd}"
        assert np.max(np.abs(out_n[1].cpu().numpy().astype(np.float64) - orew)) <= REW_TOL
        assert np.array_equal(out_n[2].cpu().numpy(), odone)
    new.check_errors(); old.check_errors()


def test_observation_against_the_oracle_300_steps():
    """the CPU oracle hands an observation out after every step (after an auto-reset: the new episode's)"""
    from control_pcgrl_amd import VecPcgrlEnv
    n = 4
    seeds = 123 + np.arange(n)
    kw = dict(change_percentage=0.02)
    env = VecPcgrlEnv("binary", "narrow", SHAPE, n, seeds=seeds, auto_reset=True, **kw)
    orc = po.OracleVecEnv("binary", "narrow", SHAPE, n, seeds=seeds, threads=2, **kw)
    _poison(env)
    obs, _ = env.reset()
    assert np.array_equal(obs.cpu().numpy().reshape(n, -1), orc.reset().reshape(n, -1)), "reset obs"
    g = torch.Generator().manual_seed(9)
    n_done = 0
    for t in range(300):
        a = torch.randint(0, env.num_actions, (n,), generator=g, dtype=torch.int32)
        _poison(env)
        obs, rew, done, _, info = env.step(a.to(env.device))
        oobs, orew, odone, ostats = orc.step(a.numpy(), auto_reset=True)
        assert np.array_equal(obs.cpu().numpy().reshape(n, -1), oobs.reshape(n, -1)), f"obs vs oracle @ {t}"
        assert np.array_equal(info["stats"].cpu().numpy(), ostats), f"stats vs oracle @ {t}"
        assert np.max(np.abs(rew.cpu().numpy().astype(np.float64) - orew)) <= REW_TOL, f"reward vs oracle @ {t}"
        assert np.array_equal(done.cpu().numpy(), odone), f"done vs oracle @ {t}"
        n_done += int(odone.sum())
    assert n_done >= n, "every env ended an episode: observations of reset maps were compared"
    env.check_errors()
