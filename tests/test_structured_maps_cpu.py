"""tests/structured_maps.py on the CPU oracle alone: the map families are what they claim to be, every morph phase reaches its
target within the steps the GPU tests give it, and the coverage floors of tests/test_gpu_structured_steps.py hold without
the engine -- a later change of the schedule cannot hollow those tests out unnoticed.  Figures of this schedule, measured
here (floor in brackets): DESIGN.md section 2, "trained-like maps"."""
import functools
import math

import numpy as np
import pytest

import paths_numpy as pn
import pcgrl_oracle as po
import structured_maps as sm

SHAPES = [(5, 5), (5, 7), (8, 8), (16, 16), (20, 24), (40, 16), (12, 40), (40, 48), (64, 64)]
BINARY = [("binary",) + form for form in sm.FORMS]
ZELDA = [("zelda",) + form for form in sm.ZELDA_FORMS]


def _ids(cases):
    return [sm.form_id(*c) for c in cases]


def _stats(grids):
    return po.stats_for_grids("binary", np.ascontiguousarray(grids))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_families_against_the_oracle_and_the_numpy_rules(shape):
    h, w = shape
    maps = {name: sm.family(name, shape) for name in sm.FAMILIES}
    st = dict(zip(maps, _stats(np.stack(list(maps.values())))))
    for name, g in maps.items():  # (the oracle and the numpy statement of the path rules agree on every family)
        assert pn.binary_path(g)[1] == st[name][1], name
    for name in ("snake_h", "snake_v", "spiral"):
        assert st[name][0] == 1, name
    assert st["snake_h"][1] >= 0.45 * h * w and st["snake_v"][1] >= 0.45 * h * w
    assert st["checker"][0] == math.ceil(h * w / 2) and st["checker"][1] == 0
    assert tuple(st["empty"]) == (1, h + w - 2) and tuple(st["solid"]) == (0, 0)
    assert tuple(st["ring"]) == (1, h + w - 2) and st["comb"][0] == 1
    # the tie: two components, and either corridor can lose an end cell without the statistic moving
    tie, k = maps["tie"], sm._half(h)
    assert st["tie"][0] == 2
    upper, lower = sm.order_from(tie, (0, 0)), sm.order_from(tie, (k + 1, 0))
    assert len(upper) == len(lower) == st["tie"][1] + 1 and not set(upper) & set(lower)
    if len(upper) > 1:
        cut = []
        for cell in (upper[0], upper[-1], lower[0], lower[-1]):
            g = tie.copy()
            g[cell] = sm.SOLID
            cut.append(g)
        assert all(tuple(s) == tuple(st["tie"]) for s in _stats(np.stack(cut)))
        assert tuple(st["off_by_one"]) == tuple(st["tie"])
        g = maps["off_by_one"].copy()  # one more cell off the upper corridor: the maximum is the lower one's, one less
        g[upper[-1]] = sm.SOLID
        assert tuple(_stats(g[None])[0]) == (2, st["tie"][1] - 1)


@pytest.mark.parametrize("shape", [(8, 8), (16, 16), (40, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_recorded_structured_maps_are_families_too(shape):
    z = np.load(sm.GOLDEN + f"/binary_{shape[0]}x{shape[1]}.npz")
    top = [sm.family(f"golden{k}", shape) for k in (0, 1)]
    assert [int(s[1]) for s in _stats(np.stack(top))] == sorted(z["L"].tolist(), reverse=True)[:2]
    assert min(int(s[1]) for s in _stats(np.stack(top))) >= 0.45 * shape[0] * shape[1]


@pytest.mark.parametrize("shape,rep", sm.ZELDA_FORMS, ids=[sm.form_id("zelda", *f) for f in sm.ZELDA_FORMS])
def test_zelda_corridor_maps_keep_one_player_key_and_door_and_a_live_path(shape, rep):
    """the maps the zelda morphs start from: one player, key and door each, up to three enemies, and the statistic is the numpy
    rules' player -> key (not through the door) plus key -> door; on the snake it is longer than the corridor"""
    h, w = shape
    n = 2 * len(sm.ZELDA_SCHEDULE)
    driver = sm.Morph("zelda", rep, shape, n, sm.FORMS[(shape, rep)]["budget"], seed=1)
    maps = driver.start_maps()
    st = po.stats_for_grids("zelda", maps)
    assert (st[:, :3] == 1).all() and st[:, 3].max() <= 3 and st[:, 3].max() > 0
    for i, m in enumerate(maps):
        p, k, d = (tuple(int(v) for v in np.argwhere(m == t)[0]) for t in (pn.PLAYER, pn.KEY, pn.DOOR))
        assert (p, d) == (driver.player, driver.door) and k == driver.key_a
        assert st[i, 6] == pn.bfs((m != pn.SOLID) & (m != pn.DOOR), p)[k] + pn.bfs(m != pn.SOLID, k)[d]
        name = sm.ZELDA_SCHEDULE[(i - 1) % len(sm.ZELDA_SCHEDULE)]
        if name in ("snake_h", "key", "walled"):
            assert st[i, 6] > st_snake(shape), (name, st[i])
    assert (st[:, 6] > 0).all()


def st_snake(shape):
    return int(_stats(sm.family("snake_h", shape)[None])[0, 1])


@functools.lru_cache(maxsize=None)
def _morph(problem, shape, rep):
    kw = sm.FORMS[(shape, rep)]
    orc = sm.make_oracle(problem, rep, shape, kw["n"])
    driver = sm.Morph(problem, rep, shape, kw["n"], kw["budget"], seed=1)
    cov = sm.Coverage(problem, shape)
    sm.run(orc, driver, kw["steps"], cov=cov)
    st = orc.get_state()
    return driver, cov, int(st["iteration"].max())


@pytest.mark.parametrize("problem,shape,rep", BINARY + ZELDA, ids=_ids(BINARY + ZELDA))
def test_morph_phases_reach_their_targets_and_meet_the_floors(problem, shape, rep):
    driver, cov, iteration = _morph(problem, shape, rep)
    kw = sm.FORMS[(shape, rep)]
    assert driver.missed == 0 and driver.completed >= kw["n"], (driver.phases, driver.completed, driver.missed)
    assert iteration <= kw["budget"] + 10  # (the restarts keep the counters far from the end of an episode)
    figures = cov.check_floors()
    assert figures["unchanged"] >= 20, figures  # (the non-changing steps take a branch of their own)
    print(sm.form_id(problem, shape, rep), figures, "phases", driver.phases, "completed", driver.completed)


@pytest.mark.parametrize("shape,rep", sm.SCRIPT_FORMS, ids=[sm.form_id("binary", *f) for f in sm.SCRIPT_FORMS])
def test_scripted_edits_do_what_their_names_say(shape, rep):
    n = 35  # five envs per script
    orc = sm.make_oracle("binary", rep, shape, n)
    driver = sm.Script(rep, shape, n)
    sm.start_script(orc, driver)
    names = [driver.scripts[i % len(driver.scripts)][0] for i in range(n)]
    start = orc.get_state()["stats"].copy()
    seen = {name: set() for name in names}
    for _ in range(sm.script_steps(shape, rep)):
        st, grids, pos = sm.oracle_state(orc)
        orc.step(driver.actions(grids, pos), want_obs=False)
        for i, s in enumerate(orc.get_state()["stats"]):
            seen[names[i]].add(tuple(int(v) for v in s))
    assert (driver.at >= [len(e) for e in driver.edits]).all()  # every env finished at least one loop
    s0 = {name: tuple(int(v) for v in start[names.index(name)]) for name in seen}
    for name, states in seen.items():
        assert s0[name] in states and len(states) >= 2, name
    r0, p0 = s0["cut_middle"]
    assert r0 == 1 and any(r == 2 and p0 // 2 - 1 <= p <= p0 // 2 + 1 for r, p in seen["cut_middle"])
    assert seen["cut_far_end"] == {(1, p0), (1, p0 - 1)} and seen["cut_first"] == {(1, p0), (1, p0 - 1)}
    (r1, p1) = s0["fill_max"]  # the pair: the maximum stays the lower corridor's once the upper one is shorter
    assert r1 == 2 and seen["fill_max"] == {(2, p1), (2, p1 - 1)}
    (r2, p2) = s0["bridge"]
    assert r2 == 2 and any(r == 1 and p > p2 for r, p in seen["bridge"])


VARIANTS = (sm.BIG_BATCH
            + [("binary", shape, rep, sm.FORMS[(shape, rep)]["n"], sm.ROLLOUT_STEPS, sm.ROLLOUT_SYNC, sm.ROLLOUT_SEED)
               for shape, rep in sorted({(s, r) for s, r, _ in sm.ROLLOUTS})]
            + [(problem, shape, rep, sm.FORMS[(shape, rep)]["n"], sm.CODES_STEPS, 10, sm.CODES_SEED) for problem, shape, rep in sm.CODES])


@pytest.mark.parametrize("problem,shape,rep,n,steps,sync,seed", VARIANTS,
                         ids=[f"{sm.form_id(*c[:3])}-{c[3]}x{c[4]}-seed{c[6]}" for c in VARIANTS])
def test_floors_of_the_shorter_gpu_runs(problem, shape, rep, n, steps, sync, seed):
    """the 1027-env runs, the recording pass of the rollout tests and the codes-form runs of the GPU file, oracle alone"""
    driver, cov = sm.Morph(problem, rep, shape, n, sm.FORMS[(shape, rep)]["budget"], seed=seed), sm.Coverage(problem, shape)
    sm.run(sm.make_oracle(problem, rep, shape, n), driver, steps, cov=cov, sync=sync)
    assert driver.missed == 0
    cov.check_floors()


@pytest.mark.parametrize("problem,shape,rep", sm.STALE_FORMS, ids=_ids(sm.STALE_FORMS))
@pytest.mark.parametrize("kind", sm.STALE_KINDS)
def test_floors_of_the_stale_mask_scenarios(kind, problem, shape, rep):
    sm.stale_scenario(kind, problem, shape, rep).check_floors()
