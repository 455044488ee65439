"""Checkpoint and restore of Super Mario Bros environments on the device (include/pcgrl_amd_smb_state.h; SmbVecEnv.state_dict /
load_state_dict / export_state / set_state / get_rng_state / set_rng_state) against the fixtures of tests/golden/smb_env, twin
envs that were never imported into, and -- under a solver budget -- the rules of tests/smb_state_rules.py launch by launch.
Every comparison is exact: float64 rewards bit for bit, observations by CRC or byte for byte, integers equal."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smb_ready_rules as RR  # noqa: E402
import smb_rules as R  # noqa: E402
import smb_state_rules as SR  # noqa: E402
import test_gpu_smb_ready as TR  # noqa: E402  (its Harness: a device env and one rules object per env in lockstep)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smb_env")
DEV = "cuda:0"
EMITTED, BUSY = RR.EMITTED, RR.BUSY


class Rules(SR.SmbReadyStateRules):
    env_class = TR.RememberingRules


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes()) & 0xFFFFFFFF


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cp = float(z["change_percentage"])
    kw = dict(representation=str(z["representation"]), map_shape=tuple(int(s) for s in z["map_shape"]),
              obs_window=tuple(int(s) for s in z["obs_window"]), weights={k: float(w) for k, w in zip(R.STAT_KEYS, z["weights"])},
              change_percentage=None if cp < 0 else cp, solver_power=int(z["solver_power"]))
    return z, kw


def make(kw, n, seeds, budget=0, **more):
    from control_pcgrl_amd import SmbReadyVecEnv, SmbVecEnv
    kw = dict(kw, **more)
    if budget:
        return SmbReadyVecEnv(num_envs=n, device=DEV, seeds=seeds, reward_dtype=torch.float64, solver_budget=budget, **kw)
    return SmbVecEnv(num_envs=n, device=DEV, seeds=seeds, reward_dtype=torch.float64, **kw)


def moments(z):
    """the three kinds of t (steps taken before the image): mid-episode, the step before an episode end, the step after one.
    The 8 x 20 fixtures end no episode within their 200 steps: three moments inside the episode there."""
    ends = np.nonzero(z["done"])[0]
    if not len(ends):
        return [1, len(z["actions"]) // 2, len(z["actions"]) - 1]
    d = int(ends[0])
    assert d >= 4 and d + 2 < len(z["actions"])
    return [d // 2, d, d + 1]


def acts(env, a):
    return torch.as_tensor(np.broadcast_to(np.asarray(a, dtype=np.int32), (env.num_envs,)).copy(), device=DEV)


def step_record(env, a):
    """one synchronous step -> everything it shows, per env: (reward, done, stats, obs crc, pos, iteration, changes)"""
    obs, rew, done, _, info = env.step(acts(env, a))
    o, r, d, s = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), info["stats"].cpu().numpy()
    st = env.get_state()
    pos, it, ch = st.pos.cpu().numpy(), st.iteration.cpu().numpy(), st.changes.cpu().numpy()
    assert r.dtype == np.float64
    return [(float(r[i]), bool(d[i]), tuple(s[i].tolist()), crc(o[i]), tuple(pos[i].tolist()), int(it[i]), int(ch[i]))
            for i in range(env.num_envs)]


def fixture_row(z, t):
    """what step_record shows of a fixture env after step t (the counters of a finished episode are gone: the new one's)"""
    ended = bool(z["done"][t])
    return (float(z["reward"][t]), ended, tuple(z["stats"][t].tolist()), int(z["obs_crc"][t]), tuple(z["pos"][t].tolist()),
            0 if ended else int(z["iteration"][t]), 0 if ended else int(z["changes"][t]))


STATE_FIELDS = ("grids", "pos", "iteration", "changes", "n_step", "searches", "stats", "last_loss", "ep_return",
                "search_iterations", "max_search_iterations")
EPISODE_FIELDS = ("ep_return", "length", "stats", "count")


def snapshot(env):
    st, le = env.get_state(), env.last_episode()
    return {f: getattr(st, f).clone() for f in STATE_FIELDS}, {f: getattr(le, f).clone() for f in EPISODE_FIELDS}


def assert_same_snapshot(a, b, rows=None, fields=STATE_FIELDS):
    for part_a, part_b, names in ((a[0], b[0], fields), (a[1], b[1], EPISODE_FIELDS)):
        for f in names:
            x, y = (part_a[f], part_b[f]) if rows is None else (part_a[f][rows], part_b[f][rows])
            assert torch.equal(x, y), f


def dirty(env, steps=7):
    """other seeds, stepped: the env's maps, records, streams and workspace are not the exporter's"""
    env.reset()
    g = torch.Generator().manual_seed(3)
    for _ in range(steps):
        env.step(torch.randint(0, env.num_actions, (env.num_envs,), generator=g, dtype=torch.int32).to(DEV))
    return env


# ------------------------------------------------------------------------------------------------- 1. continue from an image

@pytest.mark.parametrize("name", ["narrow_4x5", "turtle_5x7_cp02", "narrow_8x20_p300"])
def test_continue_from_an_image(name):
    z, kw = load(name)
    seed, actions = int(z["seed"]), z["actions"]
    a = make(kw, 3, [seed, 999, seed])
    a.reset()
    images, trace = {}, []
    for t in range(len(actions)):
        if t in moments(z):
            images[t] = a.state_dict()
        trace.append(step_record(a, actions[t]))
        assert trace[t][0] == trace[t][2] == fixture_row(z, t), t
    end = snapshot(a)
    b = dirty(make(kw, 3, [5, 6, 7]))
    for t0 in moments(z):
        sd = images[t0]
        assert sd["blob"].dtype == torch.uint8 and sd["blob"].numel() == a.state_bytes == b.state_bytes
        assert set(sd) == {"grids", "pos", "counters", "ep_return", "rng", "blob"}
        b.load_state_dict(sd)
        for t in range(t0, len(actions)):
            got = step_record(b, actions[t])
            assert got == trace[t], (t0, t)  # row 1 too; the map of the next episode proves the streams
            assert got[0] == fixture_row(z, t)
        assert_same_snapshot(snapshot(b), end)
        b.check_errors()
    a.close()
    b.close()


# --------------------------------------------------------------------------------------------------------- 2. mask and index

def test_mask_and_index():
    z, kw = load("narrow_4x5")
    n, t0, more = 65, 40, 30  # 61 steps an episode: the continuation crosses its end
    g = np.random.default_rng(1)
    plan = g.integers(0, 7, size=(t0 + more, n)).astype(np.int32)
    a = make(kw, n, np.arange(n) + 100)
    a.reset()
    for t in range(t0):
        a.step(acts(a, plan[t]))
    sd = a.state_dict()
    rest_a = [step_record(a, plan[t0 + k]) for k in range(more)]
    twin = dirty(make(kw, n, np.arange(n) + 500))
    rest_twin = [step_record(twin, plan[t0 + k]) for k in range(more)]

    def fresh():
        return dirty(make(kw, n, np.arange(n) + 500))

    # a mask: only the masked rows change
    mask = (np.arange(n) % 3 == 0)
    b = fresh()
    b.load_state_dict(sd, mask=torch.as_tensor(mask))
    for k in range(more):
        got = step_record(b, plan[t0 + k])
        for i in range(n):
            assert got[i] == (rest_a[k][i] if mask[i] else rest_twin[k][i]), (k, i)
    b.check_errors()
    b.close()
    # an index: row j continues as row index[j] of the exporter ("copy env 7 over envs 3 and 4")
    index = np.arange(n, dtype=np.int32)[::-1].copy()
    index[3] = index[4] = 7
    b = fresh()
    b.load_state_dict(sd, index=index)
    for k in range(more):
        got = step_record(b, plan[t0 + k][index])
        for j in range(n):
            assert got[j] == rest_a[k][index[j]], (k, j)
    b.check_errors()
    b.close()
    # an entry outside 0..N-1 overwrites nothing, and the error is remembered
    index = np.arange(n, dtype=np.int32)
    index[2], index[64] = n, -1
    b = fresh()
    b.load_state_dict(sd, index=index)
    with pytest.raises(ValueError, match="index entry outside"):
        b.check_errors()
    b.check_errors()  # (reported once)
    for k in range(more):
        got = step_record(b, plan[t0 + k])
        for i in range(n):
            assert got[i] == (rest_twin[k][i] if i in (2, 64) else rest_a[k][i]), (k, i)
    a.close()
    twin.close()
    b.close()


# ------------------------------------------------------------------------------------------------------- 3. parked searches

def ready_harness(name, budget, seeds):
    z, kw = load(name)
    env = make(kw, len(seeds), seeds, budget)
    rules = [Rules(seed=s, **TR.rules_kw(kw)) for s in seeds]
    actions = z["actions"]
    fixtures = {i: z for i, s in enumerate(seeds) if s == int(z["seed"])}
    h = TR.Harness(env, rules, lambda i, k: int(actions[k % len(actions)]), fixtures=fixtures, fixture_steps=len(actions),
                   check_state=False)  # (the state is compared at every launch that emits)
    return z, kw, h


def adopt(hb, ha, mask=None, index=None):
    """the harness's side of hb.env.load_state_dict(image of ha.env, mask, index): rules, progress, counters' base"""
    n = hb.n
    for j in range(n):
        if mask is not None and not mask[j]:
            continue
        src = j if index is None else int(index[j])
        SR.import_(hb.rules[j], SR.export(ha.rules[src]))
        hb.progress[j], hb.emitted[j] = ha.progress[src], ha.emitted[src]
        hb.base[j] = ha.base[src]
        if src in ha.fixtures:
            hb.fixtures[j] = ha.fixtures[src]
        else:
            hb.fixtures.pop(j, None)
    hb.largest_budget = max(hb.largest_budget, ha.largest_budget)
    hb.busy = hb.env.env_busy().cpu().numpy().astype(bool)
    assert hb.busy.tolist() == [r.busy() for r in hb.rules]
    hb._compare_state()


@pytest.mark.parametrize("name,budget,masked", [("narrow_8x20_p300", 1, False), ("turtle_8x20_p300", 3, True)])
def test_parked_searches_start_over(name, budget, masked):
    seed = int(load(name)[0]["seed"])
    z, kw, ha = ready_harness(name, budget, [seed, 999, seed, 7, 8])
    ha.reset(budget)
    # the image is taken after the first launch that leaves all three modes among the envs (the rules say which)
    while {r.mode for r in ha.rules} != {SR.IDLE, SR.PENDING_STEP, SR.PENDING_STATS}:
        ha.launch(budget)
        assert ha.launches <= 400, "no launch with all three modes: choose other seeds"
    assert sum(SR.in_flight(r) for r in ha.rules) > 0  # something is parked, past its first iteration
    sd = ha.env.state_dict()
    modes_a = [r.mode for r in ha.rules]
    # the importer: budget 3, other seeds, reset and launched twice so that searches are parked in it
    _, _, hb = ready_harness(name, 3, [11, 12, 13, 14, 15])
    hb.reset(3)
    hb.launch(3), hb.launch(3)
    mask = None
    if masked:  # row 1 keeps its own state and its own parked search
        mask = [True, False, True, True, True]
        assert hb.rules[1].busy() and SR.in_flight(hb.rules[1]) > 0
        own = (hb.rules[1].mode, hb.rules[1].remaining)
    hb.env.load_state_dict(sd, mask=None if mask is None else torch.as_tensor(mask))
    adopt(hb, ha, mask=mask)
    if masked:
        assert (hb.rules[1].mode, hb.rules[1].remaining) == own
    assert [r.mode for i, r in enumerate(hb.rules) if mask is None or mask[i]] == \
        [m for i, m in enumerate(modes_a) if mask is None or mask[i]]
    # from here on status, every emitted row, env_busy() and (at every launch that emits) the committed state equal the rules,
    # and the fixture rows emit the fixture; the synchronous env's counters are compared as the envs emit
    sync = make(kw, 5, [seed, 999, seed, 7, 8])
    sync.reset()
    sync_counters = []  # [k]: (searches, search_iterations) per env after k steps
    st = sync.get_state()
    sync_counters.append((st.searches.tolist(), st.search_iterations.tolist()))
    target = [e + 4 for e in hb.emitted]
    compared = 0
    while any(e < t for e, t in zip(hb.emitted, target)):
        status = hb.launch(3)
        assert hb.launches <= 4000, "the schedule does not advance"
        for i in range(5):
            if status[i] != EMITTED or (mask is not None and not mask[i]):
                continue  # (an env that is idle right after its step: nothing of it is in flight)
            k = hb.emitted[i]
            while len(sync_counters) <= k:
                sync.step(acts(sync, int(z["actions"][len(sync_counters) - 1])))
                st = sync.get_state()
                sync_counters.append((st.searches.tolist(), st.search_iterations.tolist()))
            st = hb.env.get_state()
            assert int(st.searches[i]) == sync_counters[k][0][i], (i, k)
            assert int(st.search_iterations[i]) == sync_counters[k][1][i], (i, k)
            compared += 1
    assert compared >= 4 and hb.seen_status >= {EMITTED, BUSY}
    hb.env.check_errors()
    for e in (ha.env, hb.env, sync):
        e.close()


# ------------------------------------------------------------------------------------------------------------------ 4. modes

def drive_ready(env, z, rows, progress, until):
    """step_ready launches that feed env i the fixture's action progress[i] when it is not busy, until the fixture rows have
    emitted the fixture up to step `until`; every emitted transition of those rows is compared with the fixture"""
    n = env.num_envs
    busy = env.env_busy().cpu().numpy().astype(bool)
    taken = list(progress)
    emitted = list(progress)
    launches = 0
    while min(emitted[i] for i in rows) < until:
        a = [int(z["actions"][taken[i] % len(z["actions"])]) for i in range(n)]
        obs, rew, done, _, info = env.step_ready(torch.tensor(a, dtype=torch.int32, device=DEV))
        launches += 1
        assert launches <= 20000
        status = info["status"].cpu().numpy()
        o, r, d, s = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), info["stats"].cpu().numpy()
        for i in range(n):
            taken[i] += int(not busy[i])
            if status[i] & EMITTED:
                t = emitted[i]
                emitted[i] += 1
                assert emitted[i] == taken[i], (i, t)
                if i in rows and t < len(z["actions"]):
                    assert (float(r[i]), bool(d[i]), tuple(s[i].tolist()), crc(o[i])) == fixture_row(z, t)[:4], (i, t)
        busy = (status & BUSY) != 0
    return emitted


def test_an_image_without_a_budget_loads_into_a_ready_env():
    z, kw = load("narrow_4x5")
    seed = int(z["seed"])
    a = make(kw, 3, [seed, 999, seed])
    a.reset()
    t0 = moments(z)[1]
    for t in range(t0):
        step_record(a, z["actions"][t])
    b = make(kw, 3, [5, 6, 7], budget=3)
    b.reset()
    for _ in range(3):
        b.step_ready(acts(b, 1))
    assert b.env_busy().any()  # searches are parked in the importer
    b.load_state_dict(a.state_dict())
    assert b.env_busy().tolist() == [0, 0, 0]  # everything idle
    drive_ready(b, z, (0, 2), [t0] * 3, len(z["actions"]))
    b.check_errors()
    a.close()
    b.close()


def test_a_busy_row_is_refused_without_a_budget_and_idle_rows_load():
    z, kw = load("narrow_4x5")
    seed = int(z["seed"])
    a = make(kw, 3, [seed, 999, seed], budget=1)
    a.reset()
    # launches until the fixture rows are idle and row 1 is busy
    progress, busy, launches = [0, 0, 0], a.env_busy().cpu().numpy().astype(bool), 0
    while not (busy.tolist() == [False, True, False] and progress[0] >= 3):
        acts_now = [int(z["actions"][p]) for p in progress]
        _, _, _, _, info = a.step_ready(torch.tensor(acts_now, dtype=torch.int32, device=DEV))
        progress = [p + int(not b) for p, b in zip(progress, busy)]
        busy = (info["status"].cpu().numpy() & BUSY) != 0
        launches += 1
        assert launches <= 3000, "rows 0 / 2 idle with row 1 busy never happens: choose another seed"
    k = progress[0]  # rows 0 and 2 have emitted k transitions and taken nothing since
    sd = a.state_dict()
    c = dirty(make(kw, 3, [5, 6, 7]))
    twin = dirty(make(kw, 3, [5, 6, 7]))
    before = c.export_state().clone()
    with pytest.raises(NotImplementedError, match="1 of the rows to import are busy"):
        c.load_state_dict(sd)
    with pytest.raises(NotImplementedError, match="busy"):
        c.load_state_dict(sd, index=[0, 1, 2], mask=[False, True, False])
    assert torch.equal(c.export_state(), before)
    c.load_state_dict(sd, mask=[True, False, True])  # the idle rows
    c.load_state_dict(sd, index=[0, 0, 2])  # row 1 from an idle row: allowed, and undone below
    c.load_state_dict({"blob": before}, mask=[False, True, False])
    for t in range(k, len(z["actions"])):
        got, want = step_record(c, z["actions"][t]), step_record(twin, z["actions"][t])
        assert got[0] == got[2] == fixture_row(z, t), t
        assert got[1] == want[1], t  # row 1 went on with its own trajectory
    for e in (a, c, twin):
        e.close()


# --------------------------------------------------------------------------------------------------------- 5. foreign images

def test_foreign_images_are_refused_and_nothing_is_overwritten():
    z, kw = load("narrow_4x5")
    target = dirty(make(kw, 3, [1, 2, 3]))
    before = target.export_state().clone()
    nbytes = target.state_bytes
    assert nbytes == 256 + 3 * (32 + 144 + 80 + 8)
    foreign = {
        "shape": make(dict(kw, map_shape=(5, 7), obs_window=(10, 14)), 3, [1, 2, 3]),
        "shape, the same bytes": make(dict(kw, map_shape=(5, 4)), 3, [1, 2, 3]),
        "representation": make(dict(kw, representation="turtle"), 3, [1, 2, 3]),
        "solver_power": make(dict(kw, solver_power=kw["solver_power"] - 1), 3, [1, 2, 3]),
        "window": make(dict(kw, obs_window=(3, 3)), 3, [1, 2, 3]),
        "weights": make(dict(kw, weights=dict(kw["weights"], enemies=kw["weights"]["enemies"] + 1.0)), 3, [1, 2, 3]),
        "change_percentage": make(dict(kw, change_percentage=0.5), 3, [1, 2, 3]),
        "batch size": make(kw, 4, [1, 2, 3, 4]),
    }
    for what, env in foreign.items():
        env.reset()
        sd = env.state_dict()
        if what in ("shape", "batch size"):
            assert sd["blob"].numel() != nbytes
        else:
            assert sd["blob"].numel() == nbytes  # only the header tells
        with pytest.raises(ValueError, match="another config"):
            target.load_state_dict(sd)
        with pytest.raises(ValueError, match="another config"):
            target.load_state_dict(sd, mask=[True, False, False])
        assert torch.equal(target.export_state(), before), what
        env.close()
    own = target.export_state().clone()
    for byte in (0, 7, 8, 15, 16, 20, 24, 28, 40, 47):  # magic, fingerprint, batch size, layout, total
        image = own.clone()
        image[byte] ^= 1
        with pytest.raises(ValueError, match="bad magic|another config"):
            target.load_state_dict({"blob": image})
        assert torch.equal(target.export_state(), before), byte
    with pytest.raises(ValueError, match="another config or batch size"):
        target.load_state_dict({"blob": own[:-8]})
    target.load_state_dict({"blob": own})  # the untouched image loads
    assert torch.equal(target.export_state(), before)
    target.close()


# ----------------------------------------------------------------------------------------------------------- 6. portable form

@pytest.mark.parametrize("name", ["narrow_4x5", "turtle_5x7_cp02"])
def test_the_portable_form_continues_the_fixture(name):
    z, kw = load(name)
    seed, actions = int(z["seed"]), z["actions"]
    a = make(kw, 3, [seed, 999, seed])
    a.reset()
    t0 = moments(z)[0]
    for t in range(t0):
        step_record(a, actions[t])
    sd = a.state_dict()
    sd.pop("blob")
    want = snapshot(a)
    b = dirty(make(kw, 3, [5, 6, 7]))
    b.load_state_dict(sd)
    got = snapshot(b)
    for f in ("grids", "pos", "iteration", "changes", "n_step", "searches", "stats", "last_loss", "ep_return"):
        assert torch.equal(got[0][f], want[0][f]), f  # statistics and last_loss recomputed from the maps: as they were
    for t in range(t0, len(actions)):
        rec_b, rec_a = step_record(b, actions[t]), step_record(a, actions[t])
        assert rec_b == rec_a and rec_b[0] == rec_b[2] == fixture_row(z, t), t
    with pytest.raises(ValueError, match="index needs the image"):
        b.load_state_dict(sd, index=[0, 1, 2])
    a.close()
    b.close()


def test_set_state_masks_clamps_and_reports_a_bad_tile():
    z, kw = load("turtle_5x7_cp02")
    a = dirty(make(kw, 3, [1, 2, 3]))
    twin = dirty(make(kw, 3, [1, 2, 3]))
    before, rng_before = snapshot(a), a.get_rng_state().clone()
    grids = torch.as_tensor(np.random.default_rng(0).integers(0, 7, size=(3, 5, 7)).astype(np.uint8), device=DEV)
    pos = torch.tensor([[-3, 99], [2, 3], [4, 6]], dtype=torch.int32, device=DEV)
    counters = torch.tensor([[5, 2, 5, 9], [1, 1, 1, 1], [7, 3, 7, 4]], dtype=torch.int32, device=DEV)
    ret = torch.tensor([1.5, -2.0, 0.25], dtype=torch.float64, device=DEV)
    a.set_state(grids, pos, counters, ret, mask=[True, False, True])
    a.check_errors()
    st = a.get_state()
    assert st.pos.tolist() == [[0, 6], before[0]["pos"][1].tolist(), [4, 6]]  # clamped, as init_pos is
    assert torch.equal(st.grids[[0, 2]], grids[[0, 2]]) and torch.equal(st.grids[1], before[0]["grids"][1])
    assert st.iteration.tolist() == [5, int(before[0]["iteration"][1]), 7] and st.searches.tolist()[0::2] == [9, 4]
    assert st.ep_return.tolist()[0::2] == [1.5, 0.25]
    # the statistics are those of a reset on the same maps
    twin.reset(init_grids=grids)
    assert torch.equal(st.stats[[0, 2]], twin.get_state().stats[[0, 2]])
    assert torch.equal(st.last_loss[[0, 2]], twin.get_state().last_loss[[0, 2]])
    # the last finished episode and the streams stay
    after = snapshot(a)
    for f in EPISODE_FIELDS:
        assert torch.equal(after[1][f], before[1][f]), f
    assert torch.equal(a.get_rng_state(), rng_before)
    assert (a.get_rng_state()[:, 8:] == 0).all()
    # the streams alone, masked
    a.set_rng_state(rng_before.roll(1, 0), mask=[False, True, False])
    now = a.get_rng_state()
    assert torch.equal(now[1], rng_before[0]) and not torch.equal(now[1], rng_before[1])
    assert torch.equal(now[0], rng_before[0]) and torch.equal(now[2], rng_before[2])
    # a tile id of 9 is read as empty and remembered
    bad = grids.clone()
    bad[2, 1, 1] = 9
    a.set_state(bad, pos, counters, ret)
    with pytest.raises(ValueError, match="tile id above 6"):
        a.check_errors()
    assert int(a.get_state().grids[2, 1, 1]) == 0
    a.close()
    twin.close()


def test_set_state_under_a_budget_leaves_envs_busy():
    z, kw = load("narrow_8x20_p300")
    seed = int(z["seed"])
    a = make(kw, 3, [seed, 999, seed])
    a.reset()
    for t in range(20):
        a.step(acts(a, z["actions"][t]))
    want = snapshot(a)
    sd = a.state_dict()
    b = make(kw, 3, [5, 6, 7], budget=1)
    b.reset()
    b.set_state(sd["grids"], sd["pos"], sd["counters"], sd["ep_return"])
    assert b.env_busy().tolist() == [1, 1, 1]
    st = b.get_state()
    assert torch.equal(st.grids, want[0]["grids"]) and torch.equal(st.searches, want[0]["searches"] - 1)
    back, busy, launches = [False] * 3, [True] * 3, 0
    while not all(back):
        _, _, _, _, info = b.step_ready(acts(b, 0))
        launches += 1
        assert launches <= 700  # two passes of 300 iterations at the most
        status = info["status"].tolist()
        st = b.get_state()
        for i in range(3):
            if busy[i] and status[i] == 0 and not back[i]:  # the statistics have arrived: reported once, before the env takes an action
                back[i] = True
                for f in ("grids", "pos", "iteration", "changes", "n_step", "searches", "stats", "last_loss", "ep_return"):
                    assert torch.equal(getattr(st, f)[i], want[0][f][i]), (i, f)
            busy[i] = bool(status[i] & BUSY)
    assert launches > 3
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------ 7. capture

def test_a_captured_step_and_export_replays_across_an_episode_end():
    z, kw = load("narrow_4x5")
    n = 3
    seeds = [int(z["seed"]), 999, 5]
    env, twin = make(kw, n, seeds), make(kw, n, seeds)
    actions = torch.zeros(n, dtype=torch.int32, device=DEV)
    out = torch.zeros(env.state_bytes, dtype=torch.uint8, device=DEV)
    env.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the usual warm-up before a capture; the env is re-seeded below
        env.step(actions)
        env.export_state(out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        env.step(actions)
        env.export_state(out)
    twin.reset()  # the twin's history is the env's: the image counts searches since the env was made
    twin.step(actions)
    for e in (env, twin):
        e.seed(seeds)
        e.reset()
    ends = 0
    for t in range(70):  # an episode is 61 steps
        actions.copy_(acts(env, z["actions"][t]))
        graph.replay()
        _, _, done, _, _ = twin.step(acts(twin, z["actions"][t]))
        ends += int(done[0])
        assert torch.equal(out, twin.export_state()), t
    assert ends == 1
    env.close()
    twin.close()


# --------------------------------------------------------------------------------------------------------------- 8. round trip

@pytest.mark.parametrize("budget", [0, 100000])
def test_import_of_the_own_export_changes_nothing(budget):
    z, kw = load("turtle_5x7_cp02")
    seeds = [int(z["seed"]), 999, 5]
    env, twin = make(kw, 3, seeds, budget), make(kw, 3, seeds, budget)
    step = (lambda e, a: e.step_ready(a)) if budget else (lambda e, a: e.step(a))
    env.reset(), twin.reset()
    for t in range(len(z["actions"])):
        if t % 7 == 3:
            env.load_state_dict(env.state_dict())
            assert torch.equal(env.export_state(), twin.export_state()), t
        a = acts(env, z["actions"][t])
        o1, r1, d1, _, i1 = step(env, a)
        o2, r2, d2, _, i2 = step(twin, a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(i1["stats"], i2["stats"]), t
        assert r1[0].item() == z["reward"][t]
    assert_same_snapshot(snapshot(env), snapshot(twin))
    env.check_errors()
    env.close()
    twin.close()
