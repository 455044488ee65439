"""Multi-agent turtle stepping (include/pcgrl_amd_multiagent.h) on the host: the rules stated in numpy
(tests/multiagent_rules.py) replay every episode recorded from the reference (tools/gen_golden_multiagent.py ->
tests/golden/multiagent/) from the seed alone, the spawn draw against numpy's own choice(replace=False), what the fixture set
has to contain, the ABI symbols, the argument checks and make_vec_env's refusals.  No GPU needed."""
import ctypes as C
import glob
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

import multiagent_rules as mr
from conftest import GOLDEN, ROOT

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "multiagent", "*.npz")))
NAMES = [os.path.basename(f)[:-4] for f in FIXTURES]


def test_fixture_set_is_complete():
    assert len(FIXTURES) == 22 and sum(os.path.getsize(f) for f in FIXTURES) < 300 * 1024
    metas = [np.load(f) for f in FIXTURES]
    shapes = {(str(z["meta_problem"]), tuple(z["meta_shape"])) for z in metas}
    for prob in ("binary", "zelda"):
        assert {(prob, s) for s in ((8, 8), (5, 7), (16, 16), (20, 24), (40, 16), (12, 40), (40, 48))} <= shapes
    assert {("binary", (1, 2)), ("binary", (2, 2))} <= shapes
    assert {int(z["meta_n_agents"]) for z in metas} == {1, 2, 3, 4, 8}
    assert {int(z["meta_show_agents"]) for z in metas} == {0, 1}
    # the kept half alternates over four consecutive resets of two agents; agents absent in some rounds
    assert any(int(z["meta_n_agents"]) == 2 and len(z["spare"]) >= 4 and z["spare"][:4, 0].tolist() in ([1, 0, 1, 0], [0, 1, 0, 1])
               for z in metas)
    assert any(((z["actions"] == -1).any(axis=1) & ~(z["actions"] == -1).all(axis=1)).any() for z in metas)


def test_fixture_set_shows_what_it_is_for():
    split = shared = both = by_changes = zelda_path = False
    for f in FIXTURES:
        z = np.load(f)
        A = int(z["meta_n_agents"])
        for acts, subs, _ in mr.fixture_rounds(z):
            if len(subs) == 0:
                continue
            d = z["done"][subs]
            # a round where one agent reports done and another steps on without
            split |= bool(d.any() and not d.all())
            r = z["reward"][subs]
            both |= bool((r < 0).any() and (r > 0).any())
        if int(z["meta_show_agents"]):
            shared |= any(len({tuple(p) for p in ps.tolist()}) < A for ps in z["pos"])
        done = z["done"].astype(bool)
        kw = mr.fixture_kwargs(z)
        cfg = mr.po.make_config(kw["problem"], "turtle", kw["map_shape"], change_percentage=kw["change_percentage"])
        by_changes |= bool((done & (z["iteration"] <= cfg.max_iterations) & (z["changes"] > cfg.max_changes)).any()) \
            if cfg.max_changes >= 0 else False
        if kw["problem"] == "zelda":
            zelda_path |= bool((z["stats"][:, 6] > 0).any())
    assert split and shared and both and by_changes and zelda_path


def test_fixture_set_shows_an_edit_that_changes_what_another_agent_sees_next():
    """in the recorded episodes themselves (the replay below ties the rules to the files): agent i changes a cell, and the
    observation agent j != i makes at its next sub-step -- the one on file, by its CRC -- shows the new tile at that cell
    inside its window, where the same window over the map without the edit does not"""
    found = 0
    for name in ("binary_8x8_a2", "zelda_8x8_a2_show", "binary_5x7_a3_show"):
        z = np.load(os.path.join(GOLDEN, "multiagent", name + ".npz"))
        rules = mr.MultiAgentRules(seed=int(z["meta_seed"]), **mr.fixture_kwargs(z))
        rules.reset()
        pending = {}  # agent -> (cell, old tile) of the latest edit by another agent
        for acts, subs, reset_after in mr.fixture_rounds(z):
            k = 0
            for i in range(rules.A):
                if acts[i] == -1 or rules.done[i]:
                    continue
                s, k = int(subs[k]), k + 1
                one = np.full(rules.A, -1, np.int32)
                one[i] = acts[i]
                before = rules.grid.copy()
                obs = rules.step(one)[0][i]
                assert mr.crc(obs) == int(z["obs_crc"][s])
                if i in pending:
                    cell, old = pending.pop(i)
                    if rules.grid[cell] != old:
                        kept, rules.grid[cell] = rules.grid[cell], old
                        without = rules.observation(i)
                        rules.grid[cell] = kept
                        y, x = cell[0] - (rules.pos[i][0] - obs.shape[0] // 2), cell[1] - (rules.pos[i][1] - obs.shape[1] // 2)
                        assert 0 <= y < obs.shape[0] and 0 <= x < obs.shape[1] and obs[y, x, 1 + kept] == 1
                        found += int(not np.array_equal(obs, without))
                if (before != rules.grid).any():
                    (cell,) = np.argwhere(before != rules.grid)
                    for j in range(rules.A):
                        if j != i and not rules.done[j]:
                            pending[j] = (tuple(cell), before[tuple(cell)])
            if reset_after:
                break
    assert found >= 10, found


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_numpy_rules_replay_the_reference(path):
    z = np.load(path)
    mr.replay_fixture(z, mr.MultiAgentRules(seed=int(z["meta_seed"]), **mr.fixture_kwargs(z)))


def test_spawn_draw_is_numpys_choice_without_replacement():
    """Floyd + shuffle on buffered 32-bit Lemire draws against Generator.choice(n, size=(A,), replace=False), three draws in
    a row on one generator so that the kept half carries over; A == n and n == 1 included"""
    cases = 0
    for seed in range(12):
        for n in (1, 2, 3, 4, 5, 7, 16, 35, 64, 256, 1920, 4096):
            for A in (1, 2, 3, 4, 8):
                if A > n:
                    continue
                bits = np.random.PCG64(np.random.SeedSequence(seed))
                ref = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))
                h32 = mr.Half32(bits)
                for _ in range(3):
                    want = ref.choice(n, size=(A,), replace=False).tolist()
                    assert mr.choice_without_replacement(h32, n, A) == want, (seed, n, A)
                    ref.random(), bits.random_raw()  # 64-bit draws in between leave the kept half alone
                st = ref.bit_generator.state
                assert (h32.has, h32.val if h32.has else 0) == (st["has_uint32"], st["uinteger"] if st["has_uint32"] else 0)
                cases += 1
    assert cases >= 300


def test_multiagent_header_symbols_exported_and_bound():
    from control_pcgrl_amd import _lib
    _lib.build()
    header = open(os.path.join(ROOT, "include", "pcgrl_amd_multiagent.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pcgrl_[a-z_]+)\s*\(", header))
    assert declared == {"pcgrl_ma_attach", "pcgrl_ma_attached", "pcgrl_ma_obs_shape", "pcgrl_ma_reset", "pcgrl_ma_step",
                        "pcgrl_ma_observe", "pcgrl_ma_get_state", "pcgrl_ma_set_state"}
    assert set(_lib.MULTIAGENT_SYMBOLS) == declared
    assert not declared & (set(_lib.SYMBOLS) | set(_lib.CODES_SYMBOLS) | set(_lib.ASYNC3D_SYMBOLS) | set(_lib.PATHS_SYMBOLS)
                           | set(_lib.SOLUTIONS_SYMBOLS))
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)
        assert fn.argtypes == _lib.MULTIAGENT_SYMBOLS[name][1] and fn.restype == _lib.MULTIAGENT_SYMBOLS[name][0], name
    for name, params in re.findall(r"\b(pcgrl_[a-z_]+)\s*\(([^)]*)\)\s*;", header):
        assert len(params.split(",")) == len(_lib.MULTIAGENT_SYMBOLS[name][1]), name
    import control_pcgrl_amd
    assert control_pcgrl_amd.__version__ == "0.7.0" and b"0.7.0" in L.pcgrl_version()


def test_multiagent_entry_points_refuse_a_null_handle_by_name():
    from control_pcgrl_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    shape, nd = (C.c_int32 * 4)(), C.c_int32()
    assert L.pcgrl_ma_attached(None) == -1
    calls = {"pcgrl_ma_attach": (None, 2, 0), "pcgrl_ma_obs_shape": (None, C.byref(shape), C.byref(nd)),
             "pcgrl_ma_reset": (None, None, None, None, p, None), "pcgrl_ma_step": (None, p, 1, p, p, p, p, p, None),
             "pcgrl_ma_observe": (None, p, None), "pcgrl_ma_get_state": (None, p, p, p, None),
             "pcgrl_ma_set_state": (None, None, p, p, p, None)}
    for name, args in calls.items():
        assert getattr(L, name)(*args) == 1, name
        assert name.encode() + b":" in L.pcgrl_last_error(), name


def _cfg(**kw):
    base = dict(representation="turtle", max_board_scans=3, change_percentage=None, n_aux_tiles=0, show_agents=False,
                controls=None, act_window=None, static_prob=None, n_static_walls=None,
                task=NS(problem="binary", map_shape=(8, 8), obs_window=(16, 16), weights=None), multiagent=NS(n_agents=2))
    base.update(kw)
    return NS(**base)


def test_make_vec_env_routes_n_agents_and_still_refuses_what_is_not_built():
    """without a GPU the multi-agent route ends in VecPcgrlEnv's 'needs a GPU' (or builds the env where there is one); it no
    longer ends in NotImplementedError.  n_aux_tiles and the combinations that are not built still do, with the reason."""
    import torch
    from control_pcgrl_amd import MultiAgentVecEnv, make_vec_env
    from control_pcgrl_amd.rllib_env import PcgrlVectorEnv
    try:
        env = make_vec_env(_cfg(), 4)
    except RuntimeError as e:
        assert not torch.cuda.is_available() and "needs a GPU" in str(e)
    else:
        assert isinstance(env, MultiAgentVecEnv) and env.n_agents == 2
        env.close()
    try:  # values that configure nothing are not refused
        make_vec_env(_cfg(controls=[], n_static_walls=0, static_prob=0, n_aux_tiles=0), 4).close()
    except RuntimeError as e:
        assert not torch.cuda.is_available() and "needs a GPU" in str(e)
    with pytest.raises(NotImplementedError, match="n_aux_tiles"):
        make_vec_env(_cfg(n_aux_tiles=3), 4)
    with pytest.raises(NotImplementedError, match="show_agents needs"):
        make_vec_env(_cfg(show_agents=True, multiagent=NS(n_agents=0)), 4)
    with pytest.raises(NotImplementedError, match="codes"):
        make_vec_env(_cfg(obs_format="codes"), 4)
    with pytest.raises(NotImplementedError, match="sub_batches"):
        make_vec_env(_cfg(), 4, sub_batches=2)
    with pytest.raises(NotImplementedError, match="Busted for now"):
        make_vec_env(_cfg(representation="narrow"), 4)
    for key, val in (("controls", ["regions"]), ("act_window", (2, 2)), ("static_prob", 0.1), ("n_static_walls", 1)):
        with pytest.raises(NotImplementedError, match=key):
            make_vec_env(_cfg(**{key: val}), 4)
    with pytest.raises(NotImplementedError, match="VectorEnv has one agent"):
        PcgrlVectorEnv(_cfg(), num_envs=4)
    with pytest.raises(ValueError, match="n_agents must be"):
        make_vec_env(_cfg(multiagent=NS(n_agents=9)), 4)
