"""The three cached planes of the binary 16x16 step -- fars, best, PREFLOOD -- held against numpy (tests/step_masks_numpy.py)
after every call, on step16_kernel, on step_kernel (PCGRL_STEP16=0) and on the codes form; and the hand-over of the PREFLOOD
plane across every call that writes, keeps or drops it (the table in DESIGN.md section 34, asserted exactly).
Run on the GPU box:  python -m pytest tests/test_gpu_step_masks.py -m gpu
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import pcgrl_oracle as po  # noqa: E402  (checker only)
import structured_maps as maps  # noqa: E402
from step16_twins import EMPTY, REW_TOL, SHAPE, _compare, _image, _pair, _same, _step_all  # noqa: E402
from step_masks_numpy import check_all  # noqa: E402
from test_gpu_step16 import _corner_cases  # noqa: E402

N = 13  # three waves and one env in a partly filled workgroup
VALID, ZERO = 1, 0


def _actions(env, g, n):
    """narrow: a tile; turtle: half moves, half tiles (a uniform turtle edits a third of the time)"""
    if env.representation == "narrow":
        return torch.randint(0, 2, (n,), generator=g, dtype=torch.int32)
    move, tile = torch.randint(0, 4, (n,), generator=g, dtype=torch.int32), torch.randint(4, 6, (n,), generator=g, dtype=torch.int32)
    return torch.where(torch.rand(n, generator=g) < 0.5, move, tile)


# ------------------------------------------------------------------------------------------------ a. after every step
@pytest.mark.parametrize("rep", ["narrow", "turtle"])
def test_masks_after_every_step_of_step16_kernel(rep):
    from control_pcgrl_amd import VecPcgrlEnv
    env = VecPcgrlEnv("binary", rep, SHAPE, N, seeds=40 + np.arange(N), auto_reset=True, change_percentage=0.05)
    env.reset()
    assert (check_all(env) == ZERO).all(), "a reset drops the PREFLOOD plane"
    g = torch.Generator().manual_seed(N)
    n_done = 0
    for t in range(120):
        out = env.step(_actions(env, g, N).to(env.device))
        n_done += int(out[2].sum())
        # a step with an observation always writes the plane, after the in-kernel reset too
        assert (check_all(env) == VALID).all(), f"PREFLOOD plane @ {t}"
    assert n_done >= N, "at least n episodes ended"
    env.check_errors()


# ------------------------------------------------------------------------------------------------ b. the corner maps
@pytest.mark.parametrize("rep", ["narrow", "turtle"])
def test_masks_on_the_injected_corner_maps_on_both_kernels(rep):
    cases = _corner_cases()
    n = len(cases)
    grids = np.stack([c[1] for c in cases])
    pos = np.array([c[2] for c in cases], np.int32)
    first = np.array([EMPTY[rep] + c[3] for c in cases], np.int32)
    seeds = 300 + np.arange(n)
    new, old = _pair(rep, n, seeds, False)
    orc = po.OracleVecEnv("binary", rep, SHAPE, n, seeds=seeds, threads=4)
    for env in (new, old):
        env.reset(init_grids=torch.as_tensor(grids), init_pos=torch.as_tensor(pos))
        assert (check_all(env) == ZERO).all()
    orc.reset(init_grids=grids, init_pos=pos)
    g = torch.Generator().manual_seed(7)
    for t in range(13):
        a = first if t == 0 else torch.randint(0, new.num_actions, (n,), generator=g, dtype=torch.int32).numpy()
        _step_all(new, old, orc, a, t, False)
        for env in (new, old):
            assert (check_all(env) == VALID).all(), t
    new.check_errors(); old.check_errors()


# ------------------------------------------------------------------------------------------------ c. the hand-overs
ROLLOUTS = [(form, want) for form in (1, 2, 0) for want in ("none", "last", "all")]
KINDS = ["step_no_obs"] + [f"rollout_{f}_{w}" for f, w in ROLLOUTS] + [
    "observe", "refresh_stats", "update_obs_refresh", "update_no_obs_refresh", "update_then_steps", "reset_masked_rng",
    "reset_masked_inject", "set_state_masked", "load_state_dict_crossed", "step_ex_reward64"]


class Trio:
    """the twins (step16_kernel, step_kernel) and the oracle through one call at a time; after every call: outputs and images
    bit-equal between the twins, the state and the outputs equal to the oracle's, every rule of the planes on both twins, and
    the PREFLOOD plane in exactly the state the table gives"""

    def __init__(self, rep):
        self.rep, seeds, kw = rep, 500 + np.arange(N), dict(change_percentage=0.05)
        self.new, self.old = _pair(rep, N, seeds, True, **kw)
        self.orc = po.OracleVecEnv("binary", rep, SHAPE, N, seeds=seeds, threads=4, **kw)
        _same(self.new.reset()[0], self.old.reset()[0], "reset obs")
        self.orc.reset()
        self.g = torch.Generator().manual_seed(17)
        self.stale = False  # pcgrl_update since the last refresh: steps take the general kernel, which drops the plane
        self.n_done = 0
        self.state = self.after("reset", ZERO)

    def actions(self, k=None):
        a = _actions(self.new, self.g, N * (k or 1))
        return a if k is None else a.reshape(k, N)

    def after(self, what, plane, dirty=0):
        """plane: VALID / ZERO for every env, or an int array [N]; dirty: envs with ENV_STATS_DIRTY (None: any number)"""
        img = _image(self.new)
        _same(img, _image(self.old), f"state image after {what}")
        maps.compare_state(self.new, self.orc, f"after {what}")
        for env in (self.new, self.old):
            state = check_all(env, img if env is self.new else None, expect_dirty=dirty)
            assert np.array_equal(state, np.broadcast_to(plane, (N,))), (what, state, plane)
        self.state = state
        return state

    def against_oracle(self, what, rew, done, stats, orew, odone, ostats):
        assert np.array_equal(stats.cpu().numpy(), ostats), f"stats vs oracle, {what}"
        assert np.max(np.abs(rew.cpu().numpy().astype(np.float64) - orew)) <= REW_TOL, f"reward vs oracle, {what}"
        assert np.array_equal(done.cpu().numpy().astype(bool), odone), f"done vs oracle, {what}"
        self.n_done += int(odone.sum())

    def step(self, what):
        """the plain observed step: VALID unless statistics may be stale (the general kernel maintains no plane)"""
        self.n_done += int(_step_all(self.new, self.old, self.orc, self.actions().numpy(), what, True).sum())
        self.after(what, ZERO if self.stale else VALID, dirty=None if self.stale else 0)

    def refresh(self, what):
        sn, so = self.new.refresh_stats(), self.old.refresh_stats()
        _same(sn, so, what)
        assert np.array_equal(sn.cpu().numpy(), self.orc.refresh_stats()), what
        self.stale = False
        self.after(what, self.state)  # map and position stand: the plane is kept as it was

    def update(self, what, want_obs):
        a = self.actions()
        on, oo = (env.update(a.to(env.device), want_obs=want_obs) for env in (self.new, self.old))
        oobs = self.orc.update(a.numpy())
        if want_obs:
            _same(on, oo, what)
            assert np.array_equal(on.cpu().numpy(), oobs), what
        self.stale = True
        self.after(what, VALID if want_obs else ZERO, dirty=None)  # (the 16x16 kernel in its update-only form)

    def call(self, kind):
        new, old, orc = self.new, self.old, self.orc
        dev = new.device
        if kind == "step_no_obs":  # pcgrl_step with d_obs = NULL (and without auto-reset: structured_maps.engine_step)
            a = self.actions()
            on, oo = (maps.engine_step(env, a.to(dev), want_obs=False) for env in (new, old))
            for k in (1, 2):
                _same(on[k], oo[k], f"{kind} output {k}")
            _same(on[4]["stats"], oo[4]["stats"], kind)
            self.against_oracle(kind, on[1], on[2], on[4]["stats"], *orc.step(a.numpy(), auto_reset=False, want_obs=False)[1:])
            self.after(kind, ZERO)
        elif kind.startswith("rollout_"):
            form, want = int(kind.split("_")[1]), kind.split("_")[2]
            a = self.actions(5)
            outs = []
            for env in (new, old):
                assert env._L.pcgrl_set_rollout_form(env._h, form) == 0
                outs.append(env.rollout(a.to(dev), want_obs=want))
                assert env._L.pcgrl_set_rollout_form(env._h, -1) == 0
            for k in range(4):
                if outs[0][k] is not None:
                    _same(outs[0][k], outs[1][k], f"{kind} output {k}")
            for k in range(5):  # a rollout is K oracle steps
                oobs, orew, odone, ostats = orc.step(a[k].numpy(), auto_reset=True, want_obs=True)
                self.against_oracle(f"{kind} step {k}", outs[0][1][k], outs[0][2][k], outs[0][3][k], orew, odone, ostats)
                if want == "all":
                    assert np.array_equal(outs[0][0][k].cpu().numpy(), oobs), f"{kind} obs {k}"
            if want == "last":
                assert np.array_equal(outs[0][0].cpu().numpy(), oobs), f"{kind} obs"
            # rollout_kernel (forms 1, 2) drops the plane; form 0 is five step launches, the last one with an observation or not
            self.after(kind, VALID if form == 0 and want != "none" else ZERO)
        elif kind == "observe":
            before = _image(new)
            on, oo = new.observe(), old.observe()
            _same(on, oo, kind)
            assert np.array_equal(on.cpu().numpy(), orc.observe()), kind
            _same(before, _image(new), "observe changes nothing")
            self.after(kind, self.state)
        elif kind == "refresh_stats":
            self.refresh(kind)
        elif kind in ("update_obs_refresh", "update_no_obs_refresh"):
            self.update(kind + ": update", kind == "update_obs_refresh")
            self.refresh(kind + ": refresh")
        elif kind == "update_then_steps":
            self.update(kind + ": update", True)
            for k in range(3):
                self.step(f"{kind}: step {k}")
            self.refresh(kind + ": refresh")
        elif kind in ("reset_masked_rng", "reset_masked_inject", "set_state_masked"):
            mask = (np.arange(N) % 3 == (0 if kind == "reset_masked_rng" else 1)).astype(np.uint8)
            st = orc.get_state()
            grids = np.roll(st["grids"].reshape((N,) + SHAPE), -1, axis=0)  # every env its neighbour's map
            pos = np.roll(st["pos"][:, :2], 2, axis=0)
            if kind == "reset_masked_rng":
                on, oo, oobs = new.reset(mask=mask)[0], old.reset(mask=mask)[0], orc.reset(mask=mask)
            elif kind == "reset_masked_inject":
                on, oo = (env.reset(mask=mask, init_grids=grids, init_pos=pos)[0] for env in (new, old))
                oobs = orc.reset(mask=mask, init_grids=grids, init_pos=pos)
            else:  # the portable form of load_state_dict: pcgrl_set_state (structured_maps.stale_scenario "set_state")
                for env in (new, old):
                    p3 = torch.zeros((N, 3), dtype=torch.int32)
                    p3[:, :2] = torch.as_tensor(pos)
                    env.load_state_dict({"grids": torch.as_tensor(grids), "pos": p3, "counters": torch.zeros((N, 4), dtype=torch.int32),
                                         "ep_return": torch.zeros(N, dtype=torch.float64), "rng": env.get_rng_state()}, mask=mask)
                on, oo, oobs = new.observe(), old.observe(), orc.reset(mask=mask, init_grids=grids, init_pos=pos)
            _same(on, oo, kind)
            assert np.array_equal(on.cpu().numpy(), oobs), kind
            self.after(kind, np.where(mask != 0, ZERO, self.state))  # per env: dropped where the call acted, kept elsewhere
        elif kind == "load_state_dict_crossed":
            sd_new, sd_old = new.state_dict(), old.state_dict()
            new.load_state_dict(sd_old)
            old.load_state_dict(sd_new)
            self.after(kind, self.state)  # the image comes with its plane
        elif kind == "step_ex_reward64":
            # float64 rewards are step_kernel's controllable-mode variant on BOTH engines (step16_kernel writes none: the
            # buffer would keep its NaNs), which maintains the plane like the plain one
            a = self.actions()
            r64 = []
            for env in (new, old):
                r64.append(torch.full((N,), float("nan"), dtype=torch.float64, device=dev))
                p, act = env._ptrs, env._actions(a.to(dev))
                assert env._L.pcgrl_step_ex(env._h, act.data_ptr(), 1, p[0], p[1], r64[-1].data_ptr(), p[2], p[3], None, env._stream()) == 0
            _compare(new, old, new._step_out, old._step_out, kind)
            _same(r64[0], r64[1], kind)
            _, orew, odone, ostats = orc.step(a.numpy(), auto_reset=True, want_obs=False)
            self.against_oracle(kind, new._reward, new._done, new._stats, orew, odone, ostats)
            assert np.max(np.abs(r64[0].cpu().numpy() - orew)) <= REW_TOL, "float64 reward vs oracle"
            _same(r64[0].to(torch.float32), new._reward, "the float64 reward rounds to the float32 reward of the same call")
            self.after(kind, VALID)
        else:
            raise AssertionError(kind)


@pytest.mark.parametrize("rep", ["narrow", "turtle"])
def test_hand_overs_of_the_preflood_plane_across_every_call(rep):
    """every call kind between two plain observed steps, twice over"""
    trio = Trio(rep)
    trio.step("first step")
    for rnd in range(2):
        for kind in KINDS:
            trio.call(kind)
            trio.step(f"step after {kind}, round {rnd}")
    assert trio.n_done >= N, "auto-resets were crossed"
    trio.new.check_errors(); trio.old.check_errors()


# ------------------------------------------------------------------------------------------------ d. the codes form
def test_masks_in_the_codes_form():
    """obs_format="codes" never routes to step16_kernel: the step launch runs without an observation (dropping the plane) and
    the codes kernel (csrc/codes/pcgrl_codes.hip) writes it after its stores"""
    from control_pcgrl_amd import VecPcgrlEnv
    env = VecPcgrlEnv("binary", "narrow", SHAPE, N, seeds=60 + np.arange(N), auto_reset=True, change_percentage=0.05, obs_format="codes")
    env.reset()
    assert (check_all(env) == VALID).all(), "reset() observes through the codes kernel"
    g = torch.Generator().manual_seed(3)
    n_done = 0
    for t in range(60):
        out = env.step(_actions(env, g, N).to(env.device))
        n_done += int(out[2].sum())
        assert (check_all(env) == VALID).all(), t
    assert n_done >= 1
    env.check_errors()
