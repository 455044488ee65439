"""The step kernels on trained-like maps (tests/structured_maps.py): corridors hundreds of cells long, components split by one
wall and merged by one opening, the maximum handed from one component to another, ties, edits on the far cell and on a
component's first cell -- the cases that decide every branch of the incremental statistics (csrc/pcgrl_kernels2d.h,
INCREMENTAL UPDATE: the cached `fars` / `best` masks, the second sweep "from the new far cells only unless a component that
attained the old maximum was touched", the replayed last trip of a long sweep) and that uniform random actions hardly ever
reach.  Engine against OracleVecEnv on every (lanes per env, mask bits) form: statistics, done and reward at every step, the
whole state and the observation every few dozen steps; through pcgrl_step, through pcgrl_rollout in its forms, in the codes
form, and across every call that could leave the cached masks stale.  change_percentage = 1.0: the change budget ends no
episode in the middle of a morph.

Every test asserts, from the ORACLE's statistics, that it was where it claims to be (structured_maps.Coverage.check_floors;
tests/test_structured_maps_cpu.py asserts the same floors without a GPU, DESIGN.md section 2 has the measured figures)."""
import numpy as np
import pytest

import structured_maps as sm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BINARY = [("binary",) + form for form in sm.FORMS]
ZELDA = [("zelda",) + form for form in sm.ZELDA_FORMS]


def _ids(cases):
    return [sm.form_id(*c) for c in cases]


def _vec(problem, rep, shape, n, **kw):
    from control_pcgrl_amd import VecPcgrlEnv
    return VecPcgrlEnv(problem, rep, shape, n, seeds=300 + np.arange(n), auto_reset=False, change_percentage=1.0, **kw)


def _pair(problem, shape, rep, n=None, seed=1, **kw):
    """(engine, oracle, morph driver, coverage, the form's steps) with the seeds of the oracle-only run"""
    form = sm.FORMS[(shape, rep)]
    n = n or form["n"]
    return (_vec(problem, rep, shape, n, **kw), sm.make_oracle(problem, rep, shape, n),
            sm.Morph(problem, rep, shape, n, form["budget"], seed=seed), sm.Coverage(problem, shape), form["steps"])


# d_obs = NULL on every step whose observation is not compared: one form per kernel family
NULL_OBS = {("binary", (16, 16), "narrow"), ("binary", (40, 48), "turtle"), ("zelda", (20, 24), "narrow")}


@pytest.mark.parametrize("problem,shape,rep", BINARY + ZELDA, ids=_ids(BINARY + ZELDA))
def test_morph_schedule_through_step(problem, shape, rep):
    """the schedule of targets through pcgrl_step, auto-reset off, phases restarted by masked reset(init_grids, init_pos);
    envs of the batch are at different points of the schedule, so a launch mixes long and short sweeps within a wave"""
    env, orc, driver, cov, steps = _pair(problem, shape, rep)
    what = sm.form_id(problem, shape, rep)
    sm.run(orc, driver, steps, env=env, cov=cov, null_obs=(problem, shape, rep) in NULL_OBS, what=what)
    assert driver.missed == 0
    print(what, cov.check_floors())
    env.close()


@pytest.mark.parametrize("problem,shape,rep,n,steps,sync,seed", sm.BIG_BATCH, ids=[c[2] for c in sm.BIG_BATCH])
def test_morph_schedule_1027_envs_on_the_16x16_kernels(problem, shape, rep, n, steps, sync, seed):
    """the compile-time kernels with several workgroups per CU; 1024 + 3 envs: the last three start a wave of their own in a
    partly filled last workgroup"""
    env, orc, driver, cov, _ = _pair(problem, shape, rep, n=n, seed=seed)
    sm.run(orc, driver, steps, env=env, cov=cov, sync=sync, obs_every=100, null_obs=rep == "narrow", what=f"{n} envs {rep}")
    print(rep, cov.check_floors())
    env.close()


@pytest.mark.parametrize("shape,rep", sm.SCRIPT_FORMS, ids=[sm.form_id("binary", *f) for f in sm.SCRIPT_FORMS])
def test_scripted_single_cell_edits(shape, rep):
    """cut a snake at its middle, at its far end and at its first row-major cell and re-open it; fill the longer corridor of a
    pair from its end until the other holds the maximum, and back; bridge and un-bridge the tie; close and open the far cell
    of a comb and of a ring -- each in a loop, 99 envs (a partly filled last wave), seven scripts side by side in a wave"""
    n = 99
    env, orc = _vec("binary", rep, shape, n), sm.make_oracle("binary", rep, shape, n)
    driver, cov = sm.Script(rep, shape, n), sm.Coverage("binary", shape)
    sm.start_script(orc, driver, env)
    sm.run(orc, driver, sm.script_steps(shape, rep), env=env, cov=cov, what=sm.form_id("binary", shape, rep))
    assert (driver.at >= [len(e) for e in driver.edits]).all()
    figures = cov.figures()
    # (every env here has a long corridor all the time; each loop of a script holds a split or a merge and a hand-over)
    assert cov.max_path >= 0.45 * shape[0] * shape[1] and 3 * cov.long >= cov.pairs, figures
    assert min(cov.split, cov.merge, cov.handover) >= 20, figures
    env.close()


def _replay(env, record, form, want_obs):
    """the recorded restarts and actions through pcgrl_rollout: one call per stretch between two restarts"""
    assert env._L.pcgrl_set_rollout_form(env._h, form) == 0
    i, t = 0, 0
    while i < len(record):
        if record[i][0] == "reset":
            _, mask, grids, pos = record[i]
            env.reset(mask=mask, init_grids=grids, init_pos=pos)
            i += 1
            continue
        j = i
        while j < len(record) and record[j][0] == "step":
            j += 1
        a = torch.as_tensor(np.stack([r[1] for r in record[i:j]])).to(env.device)
        obs, rew, done, stats = env.rollout(a, want_obs=want_obs)
        rew, done, stats = rew.cpu().numpy().astype(np.float64), done.cpu().numpy(), stats.cpu().numpy()
        for k, (_, _, orew, odone, ostats) in enumerate(record[i:j]):
            bad = np.nonzero((stats[k] != ostats).any(axis=1))[0]
            assert bad.size == 0, f"form {form} stats @ step {t + k}: envs {bad[:4]}: {stats[k][bad[:4]].tolist()} != {ostats[bad[:4]].tolist()}"
            assert np.max(np.abs(rew[k] - orew)) <= sm.REW_TOL and np.array_equal(done[k], odone), (form, t + k)
        t += j - i
        i = j
    return obs


@pytest.mark.parametrize("shape,rep,form", sm.ROLLOUTS, ids=[f"{s[0]}x{s[1]}-{r}-form{f}" for s, r, f in sm.ROLLOUTS])
def test_morph_schedule_through_rollout(shape, rep, form):
    """the same morph through pcgrl_rollout.  The driver needs the state, so an oracle-only pass records the actions, the
    restarts and the stepwise results; the engine replays them one rollout per stretch between restarts (50 steps), without
    observations and with the last one.  16 x 16: the one-launch kernel (form 1) and the two role kernels (form 2); other
    shapes have the step-launch form alone (-1)."""
    kw = sm.FORMS[(shape, rep)]
    n = kw["n"]
    orc, cov, record = sm.make_oracle("binary", rep, shape, n), sm.Coverage("binary", shape), []
    sm.run(orc, sm.Morph("binary", rep, shape, n, kw["budget"], seed=sm.ROLLOUT_SEED), sm.ROLLOUT_STEPS, cov=cov, sync=sm.ROLLOUT_SYNC,
           record=record)
    cov.check_floors()
    final = orc.observe()
    for want in ("none", "last"):
        env = _vec("binary", rep, shape, n)
        obs = _replay(env, record, form, want)
        if want == "last":
            assert np.array_equal(obs.cpu().numpy(), final)
        sm.compare_state(env, orc, f"form {form} {want}")
        env.check_errors()
        env.close()


# ---- calls that could leave `fars` / `best` stale: each mid-morph, then 50 compared steps -------------------------------------
@pytest.mark.parametrize("problem,shape,rep", sm.STALE_FORMS, ids=_ids(sm.STALE_FORMS))
@pytest.mark.parametrize("kind", sm.STALE_KINDS)
def test_cached_masks_across_state_calls(kind, problem, shape, rep):
    """structured_maps.stale_scenario: update() without refresh_stats(); state_dict() -> load_state_dict() into a second
    engine, full and masked; pcgrl_set_state; a masked inject next to wave neighbours that keep their cached masks"""
    cov = sm.stale_scenario(kind, problem, shape, rep, make_env=lambda: _vec(problem, rep, shape, sm.FORMS[(shape, rep)]["n"]))
    print(kind, sm.form_id(problem, shape, rep), cov.check_floors())


@pytest.mark.parametrize("problem,shape,rep", sm.CODES, ids=_ids(sm.CODES))
def test_morph_schedule_in_the_codes_form(problem, shape, rep):
    """obs_format="codes": the launch runs without a one-hot output and the codes are read from the state after it"""
    env, orc, driver, cov, _ = _pair(problem, shape, rep, seed=sm.CODES_SEED, obs_format="codes")
    sm.run(orc, driver, sm.CODES_STEPS, env=env, cov=cov, obs_every=20, what=f"codes {sm.form_id(problem, shape, rep)}")
    cov.check_floors()
    env.close()
