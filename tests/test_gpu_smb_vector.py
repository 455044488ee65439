"""Super Mario Bros behind the VectorEnv call shape on the device (smb_rllib.SmbVectorEnv, include/pcgrl_amd_smb_vector.h):
fixtures recorded from the reference are reproduced from the seed alone through the adapter, in both hand-out forms; the float32
hand-out kernel equals the numpy statement of tests/smb_vector_rules.py bit for bit on maps of its own, in every alignment case;
the adapter equals a twin SmbVecEnv (and the plain-Python rules of tests/smb_ctrl_rules.py) step for step with controls; nothing
handed out is written again; the direct-host and the device-block paths agree; a bad action launches nothing."""
import gc
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smb_ctrl_rules as CR  # noqa: E402
import smb_levels as sl  # noqa: E402
import smb_rules as R  # noqa: E402
import smb_vector_rules as V  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smb_env")
DEV = "cuda:0"
POWER = 300
KW57 = dict(representation="turtle", map_shape=(5, 7), obs_window=(9, 13), change_percentage=0.2, solver_power=POWER)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes()) & 0xFFFFFFFF


def make_vec(kw, n, seeds, controls=None):
    from control_pcgrl_amd import SmbVecEnv
    return SmbVecEnv(num_envs=n, device=DEV, seeds=seeds, auto_reset=False, reward_dtype=torch.float64, controls=controls, **kw)


def make_adapter(kw, n, seeds, controls=None, **adapter_kw):
    from control_pcgrl_amd import SmbVectorEnv
    return SmbVectorEnv(vec=make_vec(kw, n, seeds, controls), **adapter_kw)


def stats_of(info):
    return [info[k] for k in R.STAT_KEYS]


# -- 1. reference fixtures from the seed alone --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,steps", [("narrow_4x5", None), ("turtle_5x7_cp02", None), ("narrow_16x116", 30)])
def test_fixture_from_the_seed_alone(name, steps):
    """every sub-env of both hand-out forms reproduces the fixture; the float32 form is float32(one-hot) of the uint8 one"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cp = float(z["change_percentage"])
    kw = dict(representation=str(z["representation"]), map_shape=tuple(int(s) for s in z["map_shape"]),
              obs_window=tuple(int(s) for s in z["obs_window"]), weights={k: float(w) for k, w in zip(R.STAT_KEYS, z["weights"])},
              change_percentage=None if cp < 0 else cp, solver_power=int(z["solver_power"]))
    n, seeds = 3, [int(z["seed"])] * 3
    u8 = make_adapter(kw, n, seeds, obs_dtype=np.uint8)
    f32 = make_adapter(kw, n, seeds)
    assert f32.observation_space.shape == kw["obs_window"] + (8,) and u8.action_space.n == u8.vec.num_actions
    full = {int(t): k for k, t in enumerate(z["full_steps"])}
    ob8, infos = u8.vector_reset()
    ob32, _ = f32.vector_reset()
    assert infos == [{}] * n
    for i in range(n):
        assert ob8[i].dtype == np.uint8 and ob32[i].dtype == np.float32
        assert crc(ob8[i]) == int(z["obs0_crc"]) and np.array_equal(ob8[i], z["full_obs"][full[-1]])
        assert np.array_equal(ob32[i], ob8[i].astype(np.float32))
        for ad in (u8, f32):
            assert stats_of(ad.get_sub_environments()[i]._rep_stats) == list(z["stats0"])
    actions = z["actions"] if steps is None else z["actions"][:steps]
    ends = 0
    for t, a in enumerate(actions):
        out8 = u8.vector_step([int(a)] * n)
        out32 = f32.vector_step([int(a)] * n)
        for i in range(n):
            for ad, (obs, rew, done, trunc, infos) in ((u8, out8), (f32, out32)):
                assert isinstance(rew[i], float) and rew[i] == z["reward"][t], (t, i, rew[i], z["reward"][t])  # float64, bit for bit
                assert done[i] == bool(z["done"][t]) and trunc[i] == done[i], (t, i)
                assert stats_of(infos[i]) == z["stats"][t].tolist(), (t, i)
                assert infos[i]["iterations"] == int(z["iteration"][t]) and infos[i]["max_iterations"] == int(z["max_iterations"])
                assert infos[i]["max_changes"] == (None if int(z["max_changes"]) < 0 else int(z["max_changes"]))
            assert np.array_equal(out32[0][i], out8[0][i].astype(np.float32)), (t, i)  # (the true last one at an episode end)
            o8, o32 = out8[0][i], out32[0][i]
            if z["done"][t]:  # RLlib's reset_at; the fixture recorded the new episode's first observation
                o8, info8 = u8.reset_at(i)
                o32, _ = f32.reset_at(i)
                assert info8 == {}
                ends += i == 0
            assert crc(o8) == int(z["obs_crc"][t]), (t, i)
            assert np.array_equal(o32, o8.astype(np.float32)), (t, i)
            if t in full:
                assert np.array_equal(o8, z["full_obs"][full[t]]), (t, i)
    if name == "turtle_5x7_cp02":
        assert ends >= 1  # (max_changes ends its episodes: reset_at was on the path)
    for ad in (u8, f32):
        ad.vec.check_errors()
        ad.close()


# -- 2. the hand-out kernel against the numpy statement on own maps ----------------------------------------------------------
SHAPES = [((4, 5), (8, 10)), ((5, 7), (9, 13)), ((6, 12), (5, 9)), ((16, 116), (32, 232))]
CONTROLS = [None, ["jumps"], ["jumps", "sol-length"]]
GUARD = 8  # floats in front of and behind the image that the kernel must leave alone


def kernel_case_id(p):
    (shape, window), controls = p
    k = len(controls or [])
    return f"{shape[0]}x{shape[1]}-win{window[0]}x{window[1]}-K{k}-{V.alignment_case(k, window)}"


_CASES = [(s, c) for s in SHAPES for c in CONTROLS]


def test_the_cases_hit_every_alignment_case():
    assert {kernel_case_id(p).split("-", 3)[3] for p in _CASES} == {"Keven", "Kodd-cells-even", "Kodd-cells-odd"}


@pytest.mark.parametrize("n", [1, 3, 20, 70])
@pytest.mark.parametrize("case", _CASES, ids=kernel_case_id)
def test_hand_out_kernel_equals_the_statement(case, n):
    """positions in the four corners (the window hangs outside on every side) and one in the middle; control planes from a
    twin's ctrl_obs; the image bit for bit, into a 16-byte-aligned buffer and into one on 8 bytes only, guards untouched"""
    check_hand_out_kernel(case, n)


@pytest.mark.parametrize("case", [(SHAPES[1], ["jumps"]), (SHAPES[0], None), (SHAPES[2], ["jumps", "sol-length"])], ids=kernel_case_id)
def test_hand_out_kernel_with_one_wave_per_env(case):
    """above 1 024 envs the launcher gives every env one wave, which then makes several passes over the run even at a small
    window (5, 3 and 3 here): the form large batches run, with each alignment case once"""
    check_hand_out_kernel(case, 1100)


def check_hand_out_kernel(case, n):
    (shape, window), controls = case
    H, W = shape
    kw = dict(representation="turtle", map_shape=shape, obs_window=window, solver_power=POWER)
    grids = sl.batch(11 + H, n, H, W)
    corners = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (H // 2, W // 2)]
    pos = np.array([corners[i % 5] for i in range(n)], np.int32)
    env, twin = make_vec(kw, n, np.arange(n), controls), make_vec(kw, n, np.arange(n), controls)
    ctrl = None
    for e in (env, twin):
        if controls:  # another target per env: a plane indexed by lane or block where the env was meant shows
            e.queue_targets({k: torch.arange(n, dtype=torch.float64) * (1.5 + j) + 2.25 for j, k in enumerate(controls)})
        _, info = e.reset(init_grids=grids, init_pos=pos)
    if controls:
        ctrl = info["ctrl_obs"].cpu().numpy()  # the twin's
        assert ctrl.shape == (n, 2 * len(controls)) and len(np.unique(ctrl[:, 0])) == n
    want = V.f32_images(grids, pos, window, ctrl)
    assert want.shape == (n,) + env.obs_f32_shape
    per_env = int(np.prod(env.obs_f32_shape))
    assert env._L.pcgrl_smb_env_obs_f32_bytes(env._handle()) == per_env * 4
    for shift in (0, 2):  # floats: base on 16 bytes, and on 8 only
        buf = torch.full((GUARD + n * per_env + GUARD + 2,), -7.0, dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        ptr = buf.data_ptr() + (GUARD + shift) * 4
        assert env.observe_f32_into(ptr, env._stream()) == 0
        got = buf.cpu().numpy()
        lo, hi = GUARD + shift, GUARD + shift + n * per_env
        assert (got[:lo] == -7.0).all() and (got[hi:] == -7.0).all(), "a store outside the image"
        assert np.array_equal(got[lo:hi].reshape(want.shape), want), (shift, np.argwhere(got[lo:hi].reshape(want.shape) != want)[:4])
    with pytest.raises(ValueError, match="8-byte aligned"):
        from control_pcgrl_amd import _lib
        _lib.check(env.observe_f32_into(buf.data_ptr() + 4, env._stream()), "pcgrl_smb_env_observe_f32")
    env.check_errors()
    env.close()
    twin.close()


def test_hand_out_is_refused_under_a_solver_budget():
    from control_pcgrl_amd import SmbReadyVecEnv, SmbVectorEnv, _lib
    env = SmbReadyVecEnv("narrow", (4, 5), 2, solver_budget=64, device=DEV, obs_window=(8, 10), solver_power=POWER, auto_reset=False)
    buf = torch.zeros(2 * 8 * 10 * 8, dtype=torch.float32, device=DEV)
    with pytest.raises(NotImplementedError, match="solver budget"):
        _lib.check(env.observe_f32_into(buf.data_ptr(), env._stream()), "pcgrl_smb_env_observe_f32")
    with pytest.raises(NotImplementedError, match="synchronous"):
        SmbVectorEnv(vec=env)
    env.close()


# -- 3. against a twin, with controls ----------------------------------------------------------------------------------------
def test_adapter_equals_a_twin_with_controls():
    n, T, T_RULES = 20, 150, 40
    seeds = 300 + np.arange(n)
    ad = make_adapter(KW57, n, seeds, ["jumps"])
    twin = make_vec(KW57, n, seeds, ["jumps"])
    rules = [CR.SmbCtrlRules("turtle", (5, 7), ["jumps"], env_index=i, seed=int(seeds[i]), obs_window=(9, 13), change_percentage=0.2,
                             solver_power=POWER) for i in range(n)]
    assert ad.obs_dtype == np.float32 and ad.observation_space.shape == (9, 13, 10)
    subs = ad.get_sub_environments()
    assert subs[0].ctrl_metrics == ["jumps"] and subs[0].cond_bounds["jumps"] == twin.spec.cond_bounds["jumps"]
    static = subs[0].static_trgs["jumps"]
    rng = np.random.default_rng(5)
    new_trgs = {2: 3.0, 5: 1.5}

    def twin_images():
        st = twin.get_state()
        return V.f32_images(st.grids.cpu().numpy(), st.pos.cpu().numpy(), (9, 13), twin.ctrl_obs.cpu().numpy())

    obs, _ = ad.vector_reset()
    twin.reset()
    want = twin_images()
    for i in range(n):
        rules[i].reset()
        assert np.array_equal(obs[i], want[i])
        assert np.array_equal(obs[i][0, 0, :2], np.array(rules[i].ctrl_obs(), np.float32))
    resets_after_queue = {i: 0 for i in new_trgs}
    for t in range(T):
        if t == 20:  # mid-run, on two sub-envs: the targets wait for each env's own reset
            for i, v in new_trgs.items():
                subs[i].set_trgs({"jumps": v})
                twin.queue_targets({"jumps": v}, mask=torch.arange(n) == i)
                rules[i].set_trgs({"jumps": v})
        a = rng.integers(0, ad.action_space.n, n)
        obs, rew, done, trunc, infos = ad.vector_step(a.tolist())
        _, trew, tdone, _, tinfo = twin.step(torch.as_tensor(a, dtype=torch.int32, device=DEV))
        trew, tdone, tstats = trew.cpu().numpy(), tdone.cpu().numpy(), tinfo["stats"].cpu().numpy()
        want = twin_images()
        assert trew.dtype == np.float64
        for i in range(n):
            assert rew[i] == trew[i] and done[i] == bool(tdone[i]) and trunc[i] == done[i], (t, i)
            assert stats_of(infos[i]) == tstats[i].tolist() == stats_of(subs[i].metrics), (t, i)
            assert np.array_equal(obs[i], want[i]), (t, i)  # (the true last observation where the episode ended)
            if t < T_RULES:
                _, r_rew, r_done, r_info = rules[i].step(int(a[i]))
                assert rew[i] == r_rew and done[i] == r_done and stats_of(infos[i]) == r_info["stats"], (t, i)
                assert np.array_equal(obs[i][0, 0, :2], np.array(rules[i].ctrl_obs(), np.float32)), (t, i)
        for i, v in new_trgs.items():  # metric_trgs changes only at that env's reset
            expect = v if resets_after_queue[i] else static
            assert subs[i].metric_trgs["jumps"] == expect, (t, i)
        if any(done):
            twin.reset(mask=torch.as_tensor(tdone))
            want = twin_images()
            for i in np.nonzero(done)[0]:
                o, info = ad.reset_at(int(i))
                assert info == {} and np.array_equal(o, want[i]), (t, i)
                if t < T_RULES:
                    rules[i].reset()
                    assert np.array_equal(o[0, 0, :2], np.array(rules[i].ctrl_obs(), np.float32)), (t, i)
                if i in new_trgs and t >= 20:
                    resets_after_queue[int(i)] += 1
                    assert subs[int(i)].metric_trgs["jumps"] == new_trgs[int(i)]
    assert all(resets_after_queue.values()), "150 steps at change_percentage 0.2 end episodes in every env"
    lo = twin.get_targets().lo.cpu().numpy()[:, R.STAT_KEYS.index("jumps")]
    alo = ad.vec.get_targets().lo.cpu().numpy()[:, R.STAT_KEYS.index("jumps")]
    assert np.array_equal(lo, alo) and lo[2] == 3.0 and lo[5] == 1.5
    ad.vec.check_errors()
    ad.close()
    twin.close()


# -- 4. nothing handed out is written again -----------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_dtype,direct", [(np.float32, True), (np.float32, False), (np.uint8, None)])
def test_nothing_handed_out_is_written_again(obs_dtype, direct):
    n = 6
    ad = make_adapter(KW57, n, 40 + np.arange(n), obs_dtype=obs_dtype, direct_host_outputs=direct)
    rng = np.random.default_rng(9)
    ad.vector_reset()
    kept = []
    while len(kept) < 4:  # three consecutive steps, the third one ending an episode somewhere, and that env's reset_at
        obs, rew, done, _, infos = ad.vector_step(rng.integers(4, 11, n).tolist())
        kept.append((obs, [o.copy() for o in obs], infos, [dict(infos[i]) for i in range(n)]))
        if len(kept) == 3:
            if not any(done):
                kept.pop(0)
                continue
            o, _ = ad.reset_at(done.index(True))
            kept.append(([o], [o.copy()], infos, [dict(infos[i]) for i in range(n)]))
    def run(steps):  # (leaves no reference to anything handed out behind)
        for _ in range(steps):
            done = ad.vector_step(rng.integers(0, 11, n).tolist())[2]
            for i in np.nonzero(done)[0]:
                ad.reset_at(int(i))

    run(10)
    for live, copy, infos, info_copy in kept:
        assert all(np.array_equal(x, y) for x, y in zip(live, copy)), "a later call rewrote a returned observation"
        assert [dict(infos[i]) for i in range(n)] == info_copy, "a later call changed a returned info"
        assert live[0].dtype == np.dtype(obs_dtype)
    del kept, live, copy, infos, info_copy, obs, o
    gc.collect()
    blocks = len(ad._free)
    assert blocks >= 4
    run(30)
    gc.collect()
    assert len(ad._free) == blocks, "blocks of dropped results are recycled, none were added"
    ad.close()


# -- 5. direct-host and device-block paths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_dtype,controls", [(np.float32, None), (np.float32, ["jumps"]), (np.uint8, None)])
def test_direct_host_and_device_block_paths_agree(obs_dtype, controls):
    n, seeds = 20, 70 + np.arange(20)
    a = make_adapter(KW57, n, seeds, controls, obs_dtype=obs_dtype, direct_host_outputs=True)
    b = make_adapter(KW57, n, seeds, controls, obs_dtype=obs_dtype, direct_host_outputs=False)
    assert a._direct and a._dev is None and not b._direct
    rng = np.random.default_rng(3)
    oa, ob = a.vector_reset()[0], b.vector_reset()[0]
    assert all(np.array_equal(x, y) for x, y in zip(oa, ob))
    ends = 0
    for t in range(60):
        act = rng.integers(0, 11, n).tolist()
        ra, rb = a.vector_step(act), b.vector_step(act)
        assert all(np.array_equal(x, y) for x, y in zip(ra[0], rb[0])), t
        assert ra[1] == rb[1] and ra[2] == rb[2] and ra[3] == rb[3] and list(ra[4]) == list(rb[4]), t
        for i in np.nonzero(ra[2])[0]:
            assert np.array_equal(a.reset_at(int(i))[0], b.reset_at(int(i))[0]), (t, i)
            ends += 1
    assert ends >= 1
    a.close()
    b.close()


# -- 6. errors ---------------------------------------------------------------------------------------------------------------
def test_an_action_outside_the_space_launches_nothing():
    n = 4
    ad = make_adapter(KW57, n, 90 + np.arange(n))
    ad.vector_reset()
    ad.vector_step([4, 5, 6, 7])
    before = ad.vec.export_state().cpu().numpy()
    iters = ad._iter.copy()
    for bad in ([0, 1, 11, 2], [0, -1, 3, 2]):
        with pytest.raises(IndexError):
            ad.vector_step(bad)
    assert np.array_equal(ad.vec.export_state().cpu().numpy(), before) and np.array_equal(ad._iter, iters)
    ad.vec.check_errors()  # (the device saw no bad action either)
    ad.close()
