"""Multi-agent turtle stepping on the device (include/pcgrl_amd_multiagent.h): the reference's n_agents experiments
(configs/experiment/n_agents.yaml: representation turtle, multiagent.n_agents 1..3, show_agents on / off) -- MultiAgentWrapper
over MultiAgentTurtleRepresentation, optionally under ShowAgentRepresentation (wrappers.py:697-736, reps/wrappers.py:189-231,
:616-651).  A agents walk and edit ONE map; a round is one launch.

  MultiAgentVecEnv      the batched env: torch tensors in and out, [N, A, ...]
  MultiAgentGymEnv      one env with the reference's dict call shape (agent_i keys, '__all__')

binary and zelda; everything else the reference runs multi-agent fails in the reference itself (narrow: "Busted for now",
wide: TypeError) or is refused here with the reason (sokoban, the 3-D maze, static tiles, action patches, controls)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .vec_env import VecPcgrlEnv, _cfg_get

MAX_AGENTS = 8


class MultiAgentVecEnv:
    """N envs of A turtle agents each on one GPU.

    reset()        -> (obs uint8 [N, A, OH, OW, C], {}): every agent's window at its spawn cell; C = n_tiles + 1, and one more
                      with show_agents (the agent_occupancy plane, last)
    step(actions)  -> (obs, reward f32 [N, A], done bool [N, A], truncated = done, info); actions int32 [N, A], -1 = the agent
                      is absent this round.  info["done_all"] bool [N], info["stats"] int32 [N, A, n_stats] after each sub-step.
                      An absent or done agent takes no sub-step: reward 0, its done bit, its last statistics, and its
                      observation row keeps what it held.  One launch, no host sync.
    auto_reset=True (default): the round after which every agent is done ends with the reset inside the launch; all A
    observation rows are then the first of the new episode, and last_episode() / reduce_episodes() see the finished one
    (return = the sum over the agents, length = iteration).
    Output tensors are owned by the env and overwritten by the next call (clone to keep)."""

    def __init__(self, problem, map_shape, num_envs, n_agents, show_agents=False, device="cuda:0", obs_window=None,
                 weights=None, max_board_scans=3, change_percentage=None, seeds=None, auto_reset=True):
        n_agents = int(n_agents)
        if not 1 <= n_agents <= MAX_AGENTS:
            raise ValueError(f"n_agents must be in [1, {MAX_AGENTS}], got {n_agents}")
        self._base = VecPcgrlEnv(problem, "turtle", map_shape, num_envs, device=device, obs_window=obs_window, weights=weights,
                                 max_board_scans=max_board_scans, change_percentage=change_percentage, seeds=seeds,
                                 auto_reset=auto_reset)
        b = self._base
        # the single-agent output tensors are never written on an attached engine
        b._obs = b._reward = b._done = b._stats = b._step_out = None
        self._L, self._h = b._L, b._h
        try:
            _lib.check(self._L.pcgrl_ma_attach(self._h, n_agents, 1 if show_agents else 0), "pcgrl_ma_attach")
        except Exception:
            b.close()
            raise
        self.n_agents, self.show_agents, self.auto_reset = n_agents, bool(show_agents), bool(auto_reset)
        self.problem, self.representation, self.map_shape = problem, "turtle", b.map_shape
        self.num_envs, self.device, self.n_cells = b.num_envs, b.device, b.n_cells
        self.cfg, self.spec, self.stat_keys, self.n_stats = b.cfg, b.spec, b.stat_keys, b.n_stats
        self.num_actions, self.controls, self.obs_format = b.num_actions, [], "onehot"
        shape, nd = (C.c_int32 * 4)(), C.c_int32()
        _lib.check(self._L.pcgrl_ma_obs_shape(self._h, C.byref(shape), C.byref(nd)), "pcgrl_ma_obs_shape")
        self.obs_shape = tuple(shape[i] for i in range(nd.value))  # of ONE agent
        N, A, dev = self.num_envs, n_agents, self.device
        self._obs = torch.zeros((N, A) + self.obs_shape, dtype=torch.uint8, device=dev)
        self._reward = torch.zeros((N, A), dtype=torch.float32, device=dev)
        self._done = torch.zeros((N, A), dtype=torch.uint8, device=dev)
        self._stats = torch.zeros((N, A, self.n_stats), dtype=torch.int32, device=dev)
        self._done_all = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._ptrs = tuple(t.data_ptr() for t in (self._obs, self._reward, self._done, self._stats, self._done_all))
        done = self._done.view(torch.bool)
        self._step_out = (self._obs, self._reward, done, done, {"done_all": self._done_all.view(torch.bool), "stats": self._stats})

    # -- lifecycle ---------------------------------------------------------------------------------
    def close(self):
        self._base.close()
        self._h = None

    def seed(self, seeds):
        """Env i gets numpy PCG64(SeedSequence(seeds[i])) for both generators; the kept 32-bit half is dropped."""
        self._base.seed(seeds)

    def check_errors(self):
        """Synchronises; raises ValueError if a kernel saw an action outside {-1} + Discrete(4 + n_tiles), or a position
        outside the map."""
        self._base.check_errors()

    # -- gym-like API ------------------------------------------------------------------------------
    def _dev(self, t, dtype):
        return None if t is None else torch.as_tensor(t, device=self.device).to(dtype).contiguous()

    def reset(self, mask=None, init_grids=None, init_pos=None):
        """All envs, or those of `mask`.  init_grids uint8 [N, H, W] with init_pos int [N, A, 2] (row, col): injected maps and
        positions, which draw nothing; both or neither."""
        m, g, p = self._dev(mask, torch.uint8), self._dev(init_grids, torch.uint8), self._dev(init_pos, torch.int32)
        if g is not None and g.numel() != self.num_envs * self.n_cells:
            raise ValueError(f"init_grids must hold {self.num_envs} maps of {self.map_shape}")
        if p is not None and tuple(p.shape) != (self.num_envs, self.n_agents, 2):
            raise ValueError(f"init_pos must be [{self.num_envs}, {self.n_agents}, 2], got {tuple(p.shape)}")
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _lib.check(self._L.pcgrl_ma_reset(self._h, ptr(m), ptr(g), ptr(p), self._ptrs[0], self._base._stream()), "pcgrl_ma_reset")
        return self._obs, {}

    def step(self, actions):
        N, A = self.num_envs, self.n_agents
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions))
        if actions.numel() != N * A:
            raise ValueError(f"actions must be [{N}, {A}], got {tuple(actions.shape)}")
        if actions.dtype != torch.int32 or not actions.is_contiguous() or actions.device != self.device:
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        p = self._ptrs
        rc = self._L.pcgrl_ma_step(self._h, actions.data_ptr(), 1 if self.auto_reset else 0, p[0], p[1], p[2], p[3], p[4],
                                   self._base._stream())
        if rc:
            _lib.check(rc, "pcgrl_ma_step")
        return self._step_out

    def step_raw(self, actions_ptr, stream):
        """Lowest-overhead launch: device pointer of int32 actions [N, A] + raw hipStream_t; returns the status code."""
        p = self._ptrs
        return self._L.pcgrl_ma_step(self._h, actions_ptr, 1 if self.auto_reset else 0, p[0], p[1], p[2], p[3], p[4], stream)

    def observe(self):
        """the A observations of every env's current state (also the rows of agents that took no sub-step)"""
        _lib.check(self._L.pcgrl_ma_observe(self._h, self._ptrs[0], self._base._stream()), "pcgrl_ma_observe")
        return self._obs

    # -- state access ------------------------------------------------------------------------------
    def _side(self):
        N, A, dev = self.num_envs, self.n_agents, self.device
        pos = torch.empty((N, A, 2), dtype=torch.int32, device=dev)
        side = torch.empty((N, 4), dtype=torch.int32, device=dev)  # (uint32 words)
        last = torch.empty((N, A, _lib.PCGRL_MAX_STATS), dtype=torch.int32, device=dev)
        _lib.check(self._L.pcgrl_ma_get_state(self._h, pos.data_ptr(), side.data_ptr(), last.data_ptr(), self._base._stream()),
                   "pcgrl_ma_get_state")
        return pos, side, last

    def agent_positions(self):
        """int32 [N, A, 2]: (row, col) of every agent"""
        return self._side()[0]

    def agents_done(self):
        """bool [N, A]: the agents that have reported done since the reset"""
        bits = self._side()[1][:, 0:1]
        return ((bits >> torch.arange(self.n_agents, device=self.device, dtype=torch.int32)[None]) & 1).bool()

    def get_state(self):
        """VecPcgrlEnv.get_state() (maps, counters, statistics, loss, return; `pos` there is the wrapped turtle's own, unused
        one) plus agent_pos [N, A, 2] and agent_done [N, A]"""
        st = self._base.get_state()
        pos, side, _ = self._side()
        st.agent_pos = pos
        st.agent_done = ((side[:, 0:1] >> torch.arange(self.n_agents, device=self.device, dtype=torch.int32)[None]) & 1).bool()
        return st

    def last_episode(self):
        return self._base.last_episode()

    def reduce_episodes(self, clear=True, out=None):
        return self._base.reduce_episodes(clear=clear, out=out)

    def paths(self, cap=None, overlay=False):
        return self._base.paths(cap=cap, overlay=overlay)

    _NO_MEASURES = ("measures / diversity of a multi-agent batch: the reference computes them only in its single-agent evolution "
                    "and evaluation loops (evo/evolve.py, rl/evaluate_ctrl.py) and they are not tested here on multi-agent "
                    "engines -- hand get_state().grids to a single-agent VecPcgrlEnv's measures_for_grids / "
                    "diversity_for_grids")

    def measures(self, entropy=True):
        raise NotImplementedError(self._NO_MEASURES)

    def diversity(self, group=None, pairwise=False):
        raise NotImplementedError(self._NO_MEASURES)

    def state_dict(self):
        """The engine's state image (VecPcgrlEnv.state_dict) plus the side record: positions, done bits and the generator's kept
        half, last statistics.  A restored env continues bit-identically, also mid-episode with some agents done."""
        sd = self._base.state_dict()
        pos, side, last = self._side()
        sd["multiagent"] = {"n_agents": self.n_agents, "show_agents": self.show_agents, "pos": pos, "side": side,
                            "last_stats": last}
        return sd

    def load_state_dict(self, sd, mask=None):
        ma = sd.get("multiagent")
        if ma is None or int(ma["n_agents"]) != self.n_agents:
            raise ValueError("state_dict from an env with another number of agents (or a single-agent one)")
        base = {k: v for k, v in sd.items() if k != "multiagent"}
        if "blob" not in base:
            raise ValueError("a multi-agent state_dict carries the engine's state image ('blob')")
        self._base.load_state_dict(base, mask=mask)
        m = self._dev(mask, torch.uint8)
        pos, side, last = (self._dev(ma[k], torch.int32) for k in ("pos", "side", "last_stats"))
        N, A = self.num_envs, self.n_agents
        if tuple(pos.shape) != (N, A, 2) or tuple(side.shape) != (N, 4) or tuple(last.shape) != (N, A, _lib.PCGRL_MAX_STATS):
            raise ValueError("state_dict from an env with another batch size")
        _lib.check(self._L.pcgrl_ma_set_state(self._h, None if m is None else m.data_ptr(), pos.data_ptr(), side.data_ptr(),
                                              last.data_ptr(), self._base._stream()), "pcgrl_ma_set_state")


def make_multiagent_vec_env(cfg, num_envs, device="cuda:0", seeds=None, auto_reset=True, sub_batches=1):
    """make_vec_env(cfg, n) for cfg.multiagent.n_agents != 0 (see vec_env.make_vec_env)"""
    n_agents = int(_cfg_get(cfg, "multiagent.n_agents", 0) or 0)
    if (_cfg_get(cfg, "obs_format", "onehot") or "onehot") != "onehot":
        raise NotImplementedError("multiagent.n_agents with obs_format='codes': the multi-agent kernels write the one-hot image only")
    if int(sub_batches) > 1:
        raise NotImplementedError("multiagent.n_agents with sub_batches > 1: one engine per multi-agent batch")
    rep = _cfg_get(cfg, "representation")
    if rep != "turtle":
        raise NotImplementedError(f"multiagent.n_agents with representation '{rep}': the reference's multi-agent narrow raises "
                                  "'Busted for now' and its multi-agent wide a TypeError; turtle only")
    for key in ("controls", "act_window", "static_prob", "n_static_walls"):
        if _cfg_get(cfg, key):  # (None, 0, [] and the like configure nothing)
            raise NotImplementedError(f"multiagent.n_agents with cfg.{key}: not built (pcgrl_ma_attach refuses it)")
    return MultiAgentVecEnv(
        problem=_cfg_get(cfg, "task.problem"), map_shape=tuple(_cfg_get(cfg, "task.map_shape")), num_envs=num_envs,
        n_agents=n_agents, show_agents=bool(_cfg_get(cfg, "show_agents", False)), device=device,
        obs_window=_cfg_get(cfg, "task.obs_window"), weights=_cfg_get(cfg, "task.weights"),
        max_board_scans=_cfg_get(cfg, "max_board_scans", 3), change_percentage=_cfg_get(cfg, "change_percentage"),
        seeds=seeds, auto_reset=auto_reset)


class MultiAgentGymEnv:
    """One env with the reference's MultiAgentWrapper call shape on top of a MultiAgentVecEnv of size 1:
      reset() -> ({'agent_i': float32 [OH, OW, C]}, {})
      step({'agent_i': action}) -> obs, reward, done, truncated, info: dicts over the agents in the action dict (an agent
      left out is absent this round; one that has reported done takes no sub-step and is left out of the results), done and
      truncated with '__all__' = all of the agents in the results."""

    def __init__(self, cfg=None, vec: MultiAgentVecEnv = None, device="cuda:0", seed=None):
        self._vec = vec if vec is not None else make_multiagent_vec_env(cfg, 1, device=device, auto_reset=False,
                                                                         seeds=None if seed is None else [seed])
        assert self._vec.num_envs == 1 and not self._vec.auto_reset
        self.n_agents = self._vec.n_agents
        self.agents = [f"agent_{i}" for i in range(self.n_agents)]
        self._done = [False] * self.n_agents  # (a step() before any reset() steps the engine's initial state, as with PcgrlGymEnv)
        self._rep_stats = None

    @property
    def unwrapped(self):
        return self

    def seed(self, seed=None):
        if seed is not None:
            self._vec.seed([int(seed)])
        return [seed]

    def get_map(self):
        return self._vec.get_state().grids[0].cpu().numpy()

    def agent_positions(self):
        return self._vec.agent_positions()[0].cpu().numpy()

    def reset(self, *, seed=None, options=None):
        if seed is not None:
            self.seed(seed)
        obs, _ = self._vec.reset()
        o = obs[0].float().cpu().numpy()
        self._done = [False] * self.n_agents
        return {k: o[i] for i, k in enumerate(self.agents)}, {}

    def step(self, action):
        v = self._vec
        a = np.full((1, self.n_agents), -1, np.int32)
        for k, x in action.items():
            i = int(k.split("_")[-1])
            if not 0 <= int(x) < v.num_actions:
                raise IndexError(f"action {x} of {k} outside Discrete({v.num_actions})")
            a[0, i] = int(x)
        obs, rew, done, _, info = v.step(torch.from_numpy(a).to(v.device))
        o, r, d = obs[0].float().cpu().numpy(), rew[0].cpu().numpy(), done[0].cpu().numpy()
        st = info["stats"][0].cpu().numpy()
        out_obs, out_rew, out_done, out_info = {}, {}, {}, {}
        for k in action:
            i = int(k.split("_")[-1])
            if self._done[i]:
                continue
            out_obs[k], out_rew[k], out_done[k] = o[i], float(r[i]), bool(d[i])
            out_info[k] = {key: int(x) for key, x in zip(v.stat_keys, st[i].tolist())}
            self._rep_stats = out_info[k]
        for k in out_done:
            self._done[int(k.split("_")[-1])] = out_done[k]
        out_trunc = dict(out_done)
        out_done["__all__"] = out_trunc["__all__"] = all(out_done.values())
        return out_obs, out_rew, out_done, out_trunc, out_info

    def close(self):
        self._vec.close()
