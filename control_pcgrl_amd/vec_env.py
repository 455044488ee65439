"""Batched PCGRL environment on one MI355X: N envs advanced by one HIP launch per step.

Mirrors, for a batch, the reference's  make_env(cfg) -> ControlWrapper(CroppedImage|ActionMapImage
PCGRLWrapper(PcgrlCtrlEnv))  stack (control_pcgrl/rl/envs.py:28-81): same observation layout
(channel-last one-hot, uint8), same reward, same done rule, same per-problem stats.  All tensors live on the
env's GPU; step() performs no host synchronisation.
"""
import ctypes as C
import inspect
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .measures import MeasuresMixin
from .problems import PROBLEMS, REPRESENTATIONS, problem_spec, target_interval


def _cfg_get(cfg, path, default=None):
    cur = cfg
    for part in path.split("."):
        if cur is None:
            return default
        cur = cur.get(part, default) if isinstance(cur, dict) else getattr(cur, part, default)
    return cur


def build_config(problem, representation, map_shape, obs_window=None, weights=None, max_board_scans=3,
                 change_percentage=None, solver_power=10000, static_trgs=None, controls=None, act_window=None,
                 static_prob=None, n_static_walls=None, static_eval=False):
    """cfg fields -> pcgrl_config (include/pcgrl_amd.h)."""
    if representation not in REPRESENTATIONS:
        raise ValueError(f"Unknown representation: {representation}")  # rl/envs.py:65
    spec = problem_spec(problem, map_shape)
    map_shape = tuple(int(s) for s in map_shape)
    ndim = len(map_shape)
    if obs_window is None:
        # rl/utils.py:302-334 validate_config: default obs_window = 2 * map_shape; wide must see the whole map
        obs_window = map_shape if representation == "wide" else tuple(2 * s for s in map_shape)
    obs_window = tuple(int(s) for s in obs_window)
    weights = dict(spec.default_weights if weights is None else weights)
    trgs = dict(spec.static_trgs)
    if static_trgs:
        trgs.update(static_trgs)
    c = _lib.PcgrlConfig()
    c.problem = PROBLEMS[problem]
    c.representation = REPRESENTATIONS[representation]
    c.ndim = ndim
    for d in range(3):
        c.dims[d] = map_shape[d] if d < ndim else 1
        c.obs_window[d] = obs_window[d] if d < ndim else 1
    n_cells = int(np.prod(map_shape))
    c.max_iterations = n_cells * int(max_board_scans) + 1  # envs/pcgrl_env.py:241
    if change_percentage is None:
        c.max_changes = -1
    else:
        assert 0 < change_percentage
        c.max_changes = max(int(change_percentage * n_cells), 1)  # envs/pcgrl_env.py:235-239
    c.n_stats = len(spec.stat_keys)
    for i, k in enumerate(spec.stat_keys):
        c.weights[i] = float(weights.get(k, 0.0))  # control_wrappers.py:41-45
        if k in trgs:  # control_wrappers.py:48-82: all_metrics = static targets when not controllable
            c.has_trg[i] = 1
            c.trg_lo[i], c.trg_hi[i] = target_interval(trgs[k])
    c.solver_power = int(solver_power)
    controls = list(controls or [])
    c.n_ctrl = len(controls)
    for i, k in enumerate(controls):  # control_wrappers.py:66-73: param_ranges[k] = |bounds[1] - bounds[0]|
        if k not in spec.stat_keys or k not in spec.cond_bounds:
            raise ValueError(f"control metric '{k}' is not a metric of problem '{problem}'")
        c.ctrl_idx[i] = spec.stat_keys.index(k)
        c.ctrl_range[i] = abs(spec.cond_bounds[k][1] - spec.cond_bounds[k][0])
    if act_window is not None:  # envs/reps/wrappers.py:720-722 MultiActionRepresentation
        if len(act_window) != ndim or ndim != 2:
            raise ValueError("act_window must have one entry per map dimension (2-D problems)")
        for d in range(ndim):
            c.act_window[d] = int(act_window[d])
    # rl/utils.py:308: static_tile_wrapper = static_prob is not None or n_static_walls is not None
    if static_prob is not None or n_static_walls is not None:
        c.static_tiles = 1
        c.static_prob = float(static_prob or 0)      # envs/reps/wrappers.py:240
        c.n_static_walls = int(n_static_walls or 0)  # :242
        c.static_eval = int(bool(static_eval))
    return c, spec, obs_window


_CONFIG_ARGS = tuple(inspect.signature(build_config).parameters)[3:]  # (the keyword arguments VecPcgrlEnv hands to build_config)


# Observation forms.  "onehot" (default): the reference's image, uint8 [N, OH, OW, C] (wrappers.py:407-437 Cropped ->
# :232-257 OneHotEncoding -> :140-150 ToImage).  "codes": the same stack without OneHotEncoding, one byte per cell and plane
# (include/pcgrl_amd_codes.h): narrow / turtle [N, OH, OW, 1 + static_tiles] (0 = outside the map, 1 + tile; the static mask),
# wide [N, H, W, 1] (tile), 3-D [N, o0, o1, o2, 1] (index of the one-hot channel; 3-D wide [N, d0, d1, d2, 1]: 0 AIR, 1 DIRT,
# 2 path).  codes_to_onehot() restores the image.
OBS_FORMATS = ("onehot", "codes")
_ROLLOUT_SCRATCH_BYTES = 256 << 20  # one-hot scratch of a codes rollout that keeps every step: chunks of steps up to this size
# codes rollout(want_obs="all"), 2-D: K x (step + encoder) where the one-hot image has more bytes per cell than this, else the
# one-hot rollout + compress (profiles/obs_codes.json "rollout_all": zelda-turtle, 9 bytes per cell, 10.9 vs 26.4 us per step;
# sokoban-wide, 5 bytes, 11.2 vs 4.9 -- its one-launch rollout kernel; binary-narrow, 3 bytes, 12.2 vs 12.6)
_ROLLOUT_COMPRESS_MAX_CHANNELS = 5


def _check_obs_format(obs_format):
    if obs_format not in OBS_FORMATS:
        raise ValueError(f"obs_format must be one of {OBS_FORMATS}, got {obs_format!r}")


def obs_shape_for(cfg, spec, obs_window, obs_format="onehot"):
    """per-env observation shape of a build_config() result in either form (what pcgrl_obs_shape / pcgrl_codes_shape return)"""
    _check_obs_format(obs_format)
    nt, static = spec.n_tiles, 1 if cfg.static_tiles else 0
    if cfg.ndim == 3 and cfg.representation == REPRESENTATIONS["wide"]:  # the whole map: AIR, DIRT, path overlay
        return tuple(cfg.dims[i] for i in range(3)) + ((3,) if obs_format == "onehot" else (1,))
    if cfg.ndim == 3:
        return tuple(obs_window) + ((4,) if obs_format == "onehot" else (1,))
    if cfg.representation == REPRESENTATIONS["wide"]:
        return tuple(cfg.dims[i] for i in range(2)) + ((nt,) if obs_format == "onehot" else (1,))
    return tuple(obs_window) + ((nt + 1 + static,) if obs_format == "onehot" else (1 + static,))


def _onehot_channels(problem, representation, map_shape):
    """one-hot channels plane 0 of the codes expands to"""
    if len(tuple(map_shape)) == 3:
        return 3 if representation == "wide" else 4  # wide: obs["map"] itself (AIR, DIRT, path), nothing out of bounds
    nt = problem_spec(problem, map_shape).n_tiles
    return nt if representation == "wide" else nt + 1


def flatten_wide_action(action, map_shape, n_tiles):
    """The engine's int32 action of the wide representation from the reference's MultiDiscrete one ([..., ndim + 1] =
    cell index per axis + tile; wide_rep.py: `action[:-1]` indexes the map as it is): the C-order flat index over
    (*map_shape, n_tiles), i.e. np.ravel_multi_index(action, (*map_shape, n_tiles)).  3-D maze: (d0, d1, d2, tile).
    (The 2-D problems' flat wide action is the reference ActionMap's, which this also equals.)"""
    a = np.asarray(action, dtype=np.int64)
    dims = tuple(int(d) for d in map_shape) + (int(n_tiles),)
    if a.shape[-1] != len(dims):
        raise ValueError(f"wide action needs {len(dims)} entries per env, got shape {a.shape}")
    return np.ravel_multi_index(tuple(np.moveaxis(a, -1, 0)), dims).astype(np.int32)


def codes_high(env):
    """largest value of each codes plane (the observation_space bound): C - 1 for plane 0, 1 for the static plane"""
    c = _onehot_channels(env.problem, env.representation, env.map_shape)
    return [c - 1] + [1] * (env.obs_shape[-1] - 1)


def codes_to_onehot(codes, env):
    """The one-hot observation of `codes` (a torch tensor [..., P] in the codes form of `env`, on any device): one_hot(plane
    0, C) ++ the static plane, uint8 -- bit for bit what the env's "onehot" form shows.  `env`: anything with `problem`,
    `representation` and `map_shape` (a VecPcgrlEnv, SubBatchedVecEnv, ...).  What a policy's first layer does."""
    c = _onehot_channels(env.problem, env.representation, env.map_shape)
    codes = torch.as_tensor(codes)
    # (== F.one_hot(codes[..., 0].long(), c) without its int64 intermediate)
    oh = (codes[..., :1] == torch.arange(c, dtype=codes.dtype, device=codes.device)).to(torch.uint8)
    if codes.shape[-1] > 1:
        oh = torch.cat((oh, codes[..., 1:].to(torch.uint8)), dim=-1)
    return oh


# what follows a launch in the codes form (VecPcgrlEnv._route_obs): the codes of its observation into out_ptr
def _codes_from_state(env, out_ptr, stream):
    return env._L.pcgrl_observe_codes(env._h, out_ptr, stream)


def _codes_from_scratch(env, out_ptr, stream):
    return env._L.pcgrl_onehot_to_codes(env._h, env._via, env.num_envs, out_ptr, stream)


class VecPcgrlEnv(MeasuresMixin):
    """N independent PCGRL envs on one GPU.

    step(actions) -> (obs uint8 [N, *obs_shape], reward f32 [N], done bool [N], truncated bool [N], info)
      info["stats"]  int32 [N, n_stats] in `self.stat_keys` order
    Output tensors are owned by the env and overwritten by the next step()/reset() (clone to keep).
    obs_format="codes": every call hands out the tile-code form instead of the one-hot image (see OBS_FORMATS; the
    engine, its state and checkpoints are the same).  2-D: the call runs without a one-hot output and the codes come from
    the state after it (pcgrl_observe_codes); the 3-D maze, step_ready and rollouts that keep every step: the one-hot into
    a scratch buffer, then pcgrl_onehot_to_codes.
    auto_reset=True (default): finished envs restart inside the same launch (RLlib's convention: the returned
    observation is the first of the new episode); last_episode() exposes what RLlib's callbacks read at
    episode end (rl/callbacks.py:91-117).
    """

    def __init__(self, problem, representation, map_shape, num_envs, device="cuda:0", obs_window=None, weights=None,
                 max_board_scans=3, change_percentage=None, seeds=None, auto_reset=True, solver_power=10000,
                 static_trgs=None, controls=None, reward_dtype=torch.float32, act_window=None, static_prob=None,
                 n_static_walls=None, static_eval=False, obs_format="onehot", _out=None):
        _check_obs_format(obs_format)
        if not torch.cuda.is_available():
            raise RuntimeError("VecPcgrlEnv needs a GPU (ROCm device); there is no CPU fallback in the product path")
        self.device = torch.device(device)
        self.problem, self.representation = problem, representation
        self.map_shape = tuple(int(s) for s in map_shape)
        self.num_envs = int(num_envs)
        self.auto_reset = bool(auto_reset)
        self.cfg, self.spec, self.obs_window = build_config(
            problem, representation, map_shape, obs_window, weights, max_board_scans, change_percentage, solver_power,
            static_trgs, controls, act_window, static_prob, n_static_walls, static_eval)
        self.controls = list(controls or [])
        self.act_window = None if act_window is None else tuple(int(a) for a in act_window)
        self.static_tiles = bool(self.cfg.static_tiles)
        self.stat_keys = list(self.spec.stat_keys)
        self.n_stats = len(self.stat_keys)
        self.n_cells = int(np.prod(self.map_shape))
        L = _lib.lib()
        h = C.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(L.pcgrl_create(C.byref(self.cfg), self.num_envs, dev_index, C.byref(h)), "pcgrl_create")
        self._h = h
        self._L = L
        self._dev_index = dev_index
        shape = (C.c_int32 * 4)()
        nd = C.c_int32()
        _lib.check(L.pcgrl_obs_shape(h, C.byref(shape), C.byref(nd)), "pcgrl_obs_shape")
        self.obs_shape = tuple(shape[i] for i in range(nd.value))
        self.obs_format = obs_format
        self.onehot_shape = self.obs_shape
        if obs_format == "codes":
            _lib.check(L.pcgrl_codes_shape(h, C.byref(shape), C.byref(nd)), "pcgrl_codes_shape")
            self.obs_shape = tuple(shape[i] for i in range(nd.value))
            assert self.obs_shape == obs_shape_for(self.cfg, self.spec, self.obs_window, obs_format), self.obs_shape
        n_act = {"narrow": self.spec.n_tiles, "turtle": self.spec.n_tiles + 4,
                 "wide": self.n_cells * self.spec.n_tiles}[representation]
        self.num_actions = n_act
        # with an action patch the action is MultiDiscrete([n_tiles] * prod(act_window)): int32 [N, action_entries]
        self.action_entries = int(np.prod(self.act_window)) if self.act_window else 1
        N, dev = self.num_envs, self.device
        if _out is not None:  # SubBatchedVecEnv: this engine writes its rows of the whole batch's output tensors
            self._obs, self._reward, self._done, self._stats = _out
            assert self._obs.shape == (N,) + self.obs_shape and self._obs.is_contiguous() and self._stats.is_contiguous()
        else:
            self._obs = torch.empty((N,) + self.obs_shape, dtype=torch.uint8, device=dev)
            self._reward = torch.empty(N, dtype=torch.float32, device=dev)
            self._done = torch.empty(N, dtype=torch.uint8, device=dev)
            self._stats = torch.empty((N, self.n_stats), dtype=torch.int32, device=dev)
        self._ptrs = (self._obs.data_ptr(), self._reward.data_ptr(), self._done.data_ptr(), self._stats.data_ptr())
        self._scratch = self._status = None  # (the one-hot scratch of the codes form, step_ready's status)
        self._route_obs()
        # controllable mode / float64 rewards go through pcgrl_step_ex
        self._reward64 = torch.empty(N, dtype=torch.float64, device=dev) if reward_dtype == torch.float64 else None
        self._ctrl_obs = torch.zeros((N, 2 * len(self.controls)), dtype=torch.float32, device=dev) if self.controls else None
        self._ex = self._reward64 is not None or self._ctrl_obs is not None
        # step() hands out the same tensors every call (they are overwritten in place): the tuple is built once
        done = self._done.view(torch.bool)
        info = {"stats": self._stats}
        if self._ctrl_obs is not None:
            info["ctrl_obs"] = self._ctrl_obs
        self._step_out = (self._obs, self._reward64 if self._reward64 is not None else self._reward, done, done, info)
        if seeds is not None:
            self.seed(seeds)

    # -- lifecycle ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.pcgrl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        """raw hipStream_t of torch's current stream on the env's device (the fast accessor when this torch has it)"""
        try:
            return torch._C._cuda_getCurrentRawStream(self._dev_index)
        except AttributeError:  # pragma: no cover
            return torch.cuda.current_stream(self.device).cuda_stream

    def seed(self, seeds):
        """Env i gets numpy PCG64(SeedSequence(seeds[i])) for both RNG streams (envs/pcgrl_env.py:142-146)."""
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (self.num_envs,)))
        _lib.check(self._L.pcgrl_seed(self._h, s.ctypes.data), "pcgrl_seed")

    # -- gym-like API ------------------------------------------------------------------------------
    def reset(self, mask=None, init_grids=None, init_pos=None):
        def dev(t, dtype):
            if t is None:
                return None
            return torch.as_tensor(t, device=self.device).to(dtype).contiguous()

        m = dev(mask, torch.uint8)
        g = dev(init_grids, torch.uint8)
        p = None
        if init_pos is not None:
            ip = torch.as_tensor(init_pos, device=self.device).to(torch.int32).reshape(self.num_envs, -1)
            p = torch.zeros((self.num_envs, 3), dtype=torch.int32, device=self.device)
            p[:, : ip.shape[1]] = ip
        if g is not None:
            assert g.numel() == self.num_envs * self.n_cells
        _lib.check(self._L.pcgrl_reset(self._h, m.data_ptr() if m is not None else None,
                                       g.data_ptr() if g is not None else None,
                                       p.data_ptr() if p is not None else None, self._stream()), "pcgrl_reset")
        _lib.check(self.observe_into(self._ptrs[0], self._stream()), "pcgrl_observe")
        if self._ctrl_obs is not None:
            _lib.check(self._L.pcgrl_ctrl_observe(self._h, self._ctrl_obs.data_ptr(), self._stream()), "pcgrl_ctrl_observe")
            return self._obs, {"ctrl_obs": self._ctrl_obs}
        return self._obs, {}

    def _actions(self, actions, steps=None):
        """`actions` as the engine reads them: int32, contiguous, on the env's device, [steps x] num_envs x action_entries"""
        if actions.numel() != self.num_envs * self.action_entries * (1 if steps is None else steps):
            shape = ([steps] if steps is not None else []) + [self.num_envs] + ([self.action_entries] if self.action_entries > 1 else [])
            raise ValueError(f"actions must be {shape}, got {tuple(actions.shape)}")
        if actions.dtype != torch.int32 or not actions.is_contiguous() or actions.device != self.device:
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        return actions

    # -- the observation form: where a launch writes its observation, and what follows the launch ---------------------
    def _route_obs(self, budget=0):
        """Decides, for this env's form and solver budget, where a launch writes its observation and what then runs
        (_then) so that the observation arrives at the caller's pointer:
          one-hot                     the caller's buffer, nothing after
          codes from the state        no one-hot output, then pcgrl_observe_codes (2-D without a solver budget)
          codes through the scratch   the one-hot scratch, then pcgrl_onehot_to_codes of every row: the 3-D maze, whose
                                      observation shows the overlay of the previous statistics update, and asynchronous
                                      stepping, where the scratch keeps the rows of busy envs"""
        codes = self.obs_format == "codes"
        via_scratch = codes and (len(self.map_shape) == 3 or budget > 0)
        if via_scratch and self._scratch is None:
            self._scratch = torch.empty((self.num_envs,) + self.onehot_shape, dtype=torch.uint8, device=self.device)
        self._via = self._scratch.data_ptr() if via_scratch else None  # where launches write when _then follows them
        self._then = (_codes_from_scratch if via_scratch else _codes_from_state) if codes else None
        self._step_obs = self._ptrs[0] if self._then is None else self._via
        if via_scratch and budget > 0:  # the scratch starts as what the last call showed (nobody is busy without a budget)
            _lib.check(self._L.pcgrl_observe(self._h, self._via, self._stream()), "pcgrl_observe")

    def observe_into(self, obs_ptr, stream):
        """pcgrl_observe into a caller-given device (or mapped host) buffer, in this env's form; returns the status code"""
        then = self._then
        target = obs_ptr if then is None else self._via
        rc = self._L.pcgrl_observe(self._h, target, stream) if target is not None else 0
        if rc == 0 and then is not None:
            rc = then(self, obs_ptr, stream)
        return rc

    def step_into(self, actions_ptr, obs_ptr, reward_ptr, reward64_ptr, done_ptr, stats_ptr, ctrl_obs_ptr, stream):
        """One step launch into caller-given device (or mapped host) buffers, the observation in this env's form
        (pcgrl_step, or pcgrl_step_ex with float64 rewards or the control observation); returns the status code"""
        then, ar = self._then, 1 if self.auto_reset else 0
        obs = obs_ptr if then is None else self._via
        if reward64_ptr is None and ctrl_obs_ptr is None:
            rc = self._L.pcgrl_step(self._h, actions_ptr, ar, obs, reward_ptr, done_ptr, stats_ptr, stream)
        else:
            rc = self._L.pcgrl_step_ex(self._h, actions_ptr, ar, obs, reward_ptr, reward64_ptr, done_ptr, stats_ptr, ctrl_obs_ptr,
                                       stream)
        if rc == 0 and then is not None:
            rc = then(self, obs_ptr, stream)
        return rc

    def step(self, actions):
        # (the launch of step_into, inline: this call's host cost is what a policy-in-the-loop step pays per call)
        a, s, p = self._actions(actions).data_ptr(), self._stream(), self._ptrs
        if self._ex:
            rc = self._L.pcgrl_step_ex(self._h, a, 1 if self.auto_reset else 0, self._step_obs, p[1],
                                       self._reward64.data_ptr() if self._reward64 is not None else None, p[2], p[3],
                                       self._ctrl_obs.data_ptr() if self._ctrl_obs is not None else None, s)
        else:
            rc = self._L.pcgrl_step(self._h, a, 1 if self.auto_reset else 0, self._step_obs, p[1], p[2], p[3], s)
        if rc == 0 and self._then is not None:
            rc = self._then(self, p[0], s)
        if rc:
            _lib.check(rc, "pcgrl_step")
        return self._step_out

    # -- controllable generation (control_wrappers.py:27-121) -----------------------------------------------------
    def queue_targets(self, trgs, mask=None):
        """ControlWrapper.set_trgs: `trgs` = {metric: scalar | (lo, hi) | tensor [N]}; the targets take effect at each
        env's next reset (explicit or automatic), like the reference's _ctrl_trg_queue."""
        if not self.controls:
            raise ValueError("this env was built without `controls`")
        N, dev = self.num_envs, self.device
        lo = torch.zeros((N, self.n_stats), dtype=torch.float64, device=dev)
        hi = torch.zeros((N, self.n_stats), dtype=torch.float64, device=dev)
        for k, v in trgs.items():
            if k not in self.controls:
                raise ValueError(f"'{k}' is not a control metric of this env ({self.controls})")
            j = self.stat_keys.index(k)
            if isinstance(v, tuple):
                a, b = target_interval(v)
                lo[:, j], hi[:, j] = a, b
            else:
                t = torch.as_tensor(v, dtype=torch.float64, device=dev)
                lo[:, j] = t
                hi[:, j] = t
        m = None if mask is None else torch.as_tensor(mask, device=dev).to(torch.uint8).contiguous()
        _lib.check(self._L.pcgrl_queue_targets(self._h, m.data_ptr() if m is not None else None, lo.data_ptr(),
                                               hi.data_ptr(), self._stream()), "pcgrl_queue_targets")

    def sample_uniform_targets(self, generator=None, mask=None):
        """UniformNoiseyTargets.set_rand_trgs (control_wrappers.py:453-460): each control target ~ U(cond_bounds)."""
        trgs = {}
        for k in self.controls:
            lb, ub = self.spec.cond_bounds[k]
            u = torch.rand(self.num_envs, generator=generator, device=self.device, dtype=torch.float64)
            trgs[k] = u * (ub - lb) + lb
        self.queue_targets(trgs, mask=mask)
        return trgs

    def set_target_resampling(self, enable=True, seed=0):
        """UniformNoiseyTargets on the device (control_wrappers.py:442-471): from each env's next reset on -- explicit or
        automatic, also inside a captured HIP graph -- every control target is drawn ~ U(cond_bounds) from the env's own
        counter-based stream (pcgrl_set_target_resampling) and replaces whatever was queued.  The draw is trg_resampled
        (csrc/pcgrl_kernels2d.h)."""
        if not self.controls:
            raise ValueError("this env was built without `controls`")
        lo = np.array([self.spec.cond_bounds[k][0] for k in self.controls], dtype=np.float64)
        hi = np.array([self.spec.cond_bounds[k][1] for k in self.controls], dtype=np.float64)
        _lib.check(self._L.pcgrl_set_target_resampling(self._h, 1 if enable else 0, int(seed) & (2 ** 64 - 1),
                                                       lo.ctypes.data, hi.ctypes.data), "pcgrl_set_target_resampling")

    def sample_actions(self, seed=0, out=None):
        """action_space.sample() for every env, drawn on the device (pcgrl_sample_actions: the reference's random-action
        loops, profile_env.py:134-139): int32 [N] (or [N, prod(act_window)]), fresh at every call and at every replay of a
        HIP graph that captured the call."""
        if out is None:
            shape = (self.num_envs, self.action_entries) if self.action_entries > 1 else (self.num_envs,)
            out = torch.empty(shape, dtype=torch.int32, device=self.device)
        _lib.check(self._L.pcgrl_sample_actions(self._h, out.data_ptr(), int(seed) & (2 ** 64 - 1), self._stream()),
                   "pcgrl_sample_actions")
        return out

    def reserve_solver_pool(self, n_slots=0, allow_lazy_growth=True):
        """sokoban: size the device solver's workspace pool now (synchronous) instead of inside the first step that sees
        the solver running; n_slots 0 = full size for this batch.  Returns the slots of the pool."""
        _lib.check(self._L.pcgrl_reserve_solver_pool(self._h, int(n_slots), 1 if allow_lazy_growth else 0),
                   "pcgrl_reserve_solver_pool")
        return self.solver_pool_slots()[0]

    def solver_pool_slots(self):
        """(slots now, full size for this batch, last growth failed?)"""
        full, failed = C.c_int32(0), C.c_int32(0)
        n = int(self._L.pcgrl_solver_pool_slots(self._h, C.byref(full), C.byref(failed)))
        return n, int(full.value), bool(failed.value)

    # -- asynchronous stepping (sokoban; the 3-D maze under narrow): resumable searches behind a per-env status byte ----
    EMITTED, BUSY = 1, 2  # include/pcgrl_amd.h PCGRL_ENV_EMITTED / PCGRL_ENV_BUSY

    def set_solver_budget(self, budget):
        """budget > 0: the device solver works to `budget` iteration units per env and launch and parks what it could not
        finish; step with step_ready() from here on (step() / rollout() / update() are refused).  0: synchronous again.
        In the reference a slow _run_game (sokoban_prob.py:99-148) stalls one env, not the fleet (rl/utils.py:412-415).
        minecraft_3D_maze under narrow: `budget` = trips of the path search per env and launch (include/pcgrl_amd_async3d.h)."""
        _lib.check(self._L.pcgrl_set_solver_budget(self._h, int(budget)), "pcgrl_set_solver_budget")
        if budget > 0 and self._status is None:
            self._status = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
            info = dict(self._step_out[4], status=self._status)
            self._ready_out = self._step_out[:4] + (info,)
        self._route_obs(budget)

    def step_ready(self, actions):
        """pcgrl_step_ready: like step(), plus info["status"] uint8 [N] = EMITTED (this env completed a step in this launch:
        its reward / done / stats / obs rows are valid) | BUSY (a search of its level is parked: it ignores the NEXT call's
        action).  An env consumes the action of a call iff it was not busy after the previous one; an emitted transition
        belongs to the last action the env consumed.  The reward / done / stats rows of envs that did not emit keep their
        previous contents; their obs rows are rewritten with the observation of the step in flight."""
        if self._status is None:
            raise ValueError("step_ready needs a solver budget: call set_solver_budget(budget > 0) first")
        rc = self.step_ready_raw(self._actions(actions).data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            _lib.check(rc, "pcgrl_step_ready")
        return self._ready_out

    def step_ready_raw(self, actions_ptr, status_ptr, stream):
        p = self._ptrs
        rc = self._L.pcgrl_step_ready(self._h, actions_ptr, 1 if self.auto_reset else 0, self._step_obs, p[1], p[2], p[3],
                                      status_ptr, stream)
        if rc == 0 and self._then is not None:
            rc = self._then(self, p[0], stream)
        return rc

    def env_busy(self):
        """uint8 [N]: 1 = the env waits for a parked search (after reset(): which envs will ignore the first action)"""
        out = torch.empty(self.num_envs, dtype=torch.uint8, device=self.device)
        _lib.check(self._L.pcgrl_env_busy(self._h, out.data_ptr(), self._stream()), "pcgrl_env_busy")
        return out

    def step_raw(self, actions_ptr, stream):
        """Lowest-overhead launch: device pointer of int32 actions + raw hipStream_t."""
        p = self._ptrs
        rc = self._L.pcgrl_step(self._h, actions_ptr, 1 if self.auto_reset else 0, self._step_obs, p[1], p[2], p[3], stream)
        if rc == 0 and self._then is not None:
            rc = self._then(self, p[0], stream)
        return rc

    def step_seq_raw(self, rows_ptr, row_stride, n_rows, first_row, n_steps, stream):
        """n_steps pcgrl_step launches from ONE foreign call (pcgrl_step_seq): step k uses action row
        (first_row + k) % n_rows of the int32 buffer at rows_ptr (rows row_stride entries apart)."""
        if self._then is not None:  # (a launch follows every step: two launches per step)
            for k in range(n_steps):
                rc = self.step_raw(rows_ptr + 4 * ((first_row + k) % n_rows) * row_stride, stream)
                if rc:
                    return rc
            return 0
        return self._L.pcgrl_step_seq(self._h, rows_ptr, row_stride, n_rows, first_row, n_steps, 1 if self.auto_reset else 0,
                                      self._ptrs[0], self._ptrs[1], self._ptrs[2], self._ptrs[3], stream)

    def rollout(self, actions, want_obs="all"):
        """Open-loop rollout: `actions` int32 [K, N] (or [K, N, prod(act_window)] with an action patch); K steps in one
        launch (pcgrl_rollout / pcgrl_rollout_ex).  Returns (obs, reward [K, N], done [K, N], stats [K, N, n_stats]); obs
        is [K, N, ...] for want_obs="all", [N, ...] (after the last step) for "last", None for "none".  Fresh tensors, not
        the env's step buffers.  Controllable mode: rewards are float64 and `self.ctrl_obs` holds the control observation
        after the last step.
        In the codes form, "last" and "none" take the launch path of step(); "all" either runs K x (step launch without an
        observation + encoder into row k), for 2-D images of more than _ROLLOUT_COMPRESS_MAX_CHANNELS bytes per cell, or
        the rollout in chunks of steps whose one-hot observations fit a scratch of <= _ROLLOUT_SCRATCH_BYTES (at least one
        step), each chunk compressed into its rows of the result.  Chunks of one rollout give the results of the whole
        (pcgrl_rollout's definition: n_steps pcgrl_step calls), and every chunk keeps the engine's rollout form."""
        if want_obs not in ("all", "last", "none"):
            raise ValueError(f"want_obs must be 'all', 'last' or 'none', got {want_obs!r}")
        K = int(actions.shape[0])
        actions = self._actions(actions, K)
        N, dev, s = self.num_envs, self.device, self._stream()
        obs = None if want_obs == "none" else torch.empty(((K, N) if want_obs == "all" else (N,)) + self.obs_shape,
                                                          dtype=torch.uint8, device=dev)
        rew = torch.empty((K, N), dtype=torch.float32, device=dev)
        rew64 = torch.empty((K, N), dtype=torch.float64, device=dev) if self._reward64 is not None else None
        done = torch.empty((K, N), dtype=torch.uint8, device=dev)
        stats = torch.empty((K, N, self.n_stats), dtype=torch.int32, device=dev)
        ctrl = self._ctrl_obs.data_ptr() if self._ctrl_obs is not None else None
        out = obs, (rew64 if rew64 is not None else rew), done.view(torch.bool), stats

        def rows(k):  # pointers of the outputs from step k on
            return rew[k].data_ptr(), None if rew64 is None else rew64[k].data_ptr(), done[k].data_ptr(), stats[k].data_ptr()

        L, h, ar, act = self._L, self._h, 1 if self.auto_reset else 0, actions.reshape(K, -1)
        if want_obs == "all" and self._then is _codes_from_state and self.onehot_shape[-1] > _ROLLOUT_COMPRESS_MAX_CHANNELS:
            for k in range(K):  # (pcgrl_rollout's own definition: K pcgrl_step calls)
                _lib.check(self.step_into(act[k].data_ptr(), obs[k].data_ptr(), *rows(k), ctrl if k == K - 1 else None, s),
                           "pcgrl_step_ex")
        elif want_obs == "all" and self._then is not None:
            kc = max(1, min(K, _ROLLOUT_SCRATCH_BYTES // (N * int(np.prod(self.onehot_shape)))))
            scratch = torch.empty((kc, N) + self.onehot_shape, dtype=torch.uint8, device=dev)
            for k0 in range(0, K, kc):
                kk = min(kc, K - k0)
                _lib.check(L.pcgrl_rollout_ex(h, act[k0].data_ptr(), kk, ar, scratch.data_ptr(), 0, *rows(k0),
                                              ctrl if k0 + kk == K else None, s), "pcgrl_rollout_ex")
                _lib.check(L.pcgrl_onehot_to_codes(h, scratch.data_ptr(), kk * N, obs[k0].data_ptr(), s), "pcgrl_onehot_to_codes")
        else:
            target = None if obs is None else obs.data_ptr() if self._then is None else self._via
            rc = L.pcgrl_rollout_ex(h, actions.data_ptr(), K, ar, target, 1 if want_obs == "last" else 0, *rows(0), ctrl, s)
            if rc == 0 and obs is not None and self._then is not None:
                rc = self._then(self, obs.data_ptr(), s)
            _lib.check(rc, "pcgrl_rollout_ex")
        return out

    @property
    def ctrl_obs(self):
        """float32 [N, 2 * len(controls)]: (target / range, metric / range) per control metric, as of the last step"""
        return self._ctrl_obs

    # -- evolution-driver pattern (evo/evolve.py:1083-1120): rep.update() many times, get_stats() once ---------------
    def update(self, actions, want_obs=True):
        """rep.update(action) for every env (+ observation); counters / stats / reward are untouched."""
        a, s = self._actions(actions).data_ptr(), self._stream()
        rc = self._L.pcgrl_update(self._h, a, self._step_obs if want_obs else None, s)
        if rc == 0 and want_obs and self._then is not None:
            rc = self._then(self, self._ptrs[0], s)
        _lib.check(rc, "pcgrl_update")
        return self._obs if want_obs else None

    def refresh_stats(self):
        """Problem.get_stats() of the current maps; returns int32 [N, n_stats]."""
        _lib.check(self._L.pcgrl_refresh_stats(self._h, self._ptrs[3], self._stream()), "pcgrl_refresh_stats")
        return self._stats

    def observe(self):
        _lib.check(self.observe_into(self._ptrs[0], self._stream()), "pcgrl_observe")
        return self._obs

    # -- static tiles (envs/reps/wrappers.py:234-376) ---------------------------------------------------------------
    def get_static(self):
        """StaticTileRepresentation.static_tiles, uint8 [N, H+2, W+2] (bordered layout, border ring = 1)."""
        if not self.static_tiles:
            raise ValueError("this env was built without static tiles")
        h, w = self.map_shape
        out = torch.empty((self.num_envs, h + 2, w + 2), dtype=torch.uint8, device=self.device)
        _lib.check(self._L.pcgrl_get_static(self._h, out.data_ptr(), self._stream()), "pcgrl_get_static")
        return out

    def set_static(self, static_prob=None, n_static_walls=None, eval_mode=None):
        """set_static_prob / set_n_static_walls / set_eval_mode (:256-263; rl/evaluate.py:128-129); next reset on.  None
        leaves a value as the engine holds it (also after load_state_dict of a checkpoint taken in another mode)."""
        _lib.check(self._L.pcgrl_set_static(self._h, -1.0 if static_prob is None else float(static_prob),
                                            -1 if n_static_walls is None else int(n_static_walls),
                                            -1 if eval_mode is None else int(bool(eval_mode))), "pcgrl_set_static")

    def check_errors(self):
        """Synchronises; raises ValueError if a kernel saw an action outside the action space."""
        _lib.check(self._L.pcgrl_poll_error(self._h), "pcgrl_poll_error")

    # -- state access ------------------------------------------------------------------------------
    def get_state(self):
        N, dev = self.num_envs, self.device
        out = SimpleNamespace(
            grids=torch.empty((N,) + self.map_shape, dtype=torch.uint8, device=dev),
            pos=torch.empty((N, 3), dtype=torch.int32, device=dev),
            counters=torch.empty((N, 4), dtype=torch.int32, device=dev),
            stats=torch.empty((N, self.n_stats), dtype=torch.int32, device=dev),
            last_loss=torch.empty(N, dtype=torch.float64, device=dev),
            ep_return=torch.empty(N, dtype=torch.float64, device=dev))
        _lib.check(self._L.pcgrl_get_state(self._h, out.grids.data_ptr(), out.pos.data_ptr(), out.counters.data_ptr(),
                                           out.stats.data_ptr(), out.last_loss.data_ptr(), out.ep_return.data_ptr(),
                                           self._stream()), "pcgrl_get_state")
        out.iteration, out.changes, out.n_step, out.ep_len = (out.counters[:, i] for i in range(4))
        return out

    def last_episode(self):
        N, dev = self.num_envs, self.device
        out = SimpleNamespace(ep_return=torch.empty(N, dtype=torch.float64, device=dev),
                              ep_len=torch.empty(N, dtype=torch.int32, device=dev),
                              final_stats=torch.empty((N, self.n_stats), dtype=torch.int32, device=dev),
                              n_episodes=torch.empty(N, dtype=torch.int64, device=dev))
        _lib.check(self._L.pcgrl_get_last_episode(self._h, out.ep_return.data_ptr(), out.ep_len.data_ptr(),
                                                  out.final_stats.data_ptr(), out.n_episodes.data_ptr(),
                                                  self._stream()), "pcgrl_get_last_episode")
        return out

    def stats_for_grids(self, grids):
        """Problem.get_stats on caller maps (the evolution driver's entry, evo/evolve.py:1083-1120).  Any number of
        maps; asynchronous (uses this engine's scratch; device-side errors surface in check_errors())."""
        g = torch.as_tensor(grids, device=self.device).to(torch.uint8).contiguous()
        n = g.numel() // self.n_cells
        out = torch.empty((n, self.n_stats), dtype=torch.int32, device=self.device)
        _lib.check(self._L.pcgrl_stats_for_grids_h(self._h, n, g.data_ptr(), out.data_ptr(), self._stream()),
                   "pcgrl_stats_for_grids_h")
        return out

    # -- solution paths (include/pcgrl_amd_paths.h) ------------------------------------------------------------------
    def _paths(self, n, grids, cap, overlay):
        if cap is None:  # (a problem without paths reports 0: the call below is what refuses it)
            cap = max(1, int(self._L.pcgrl_path_capacity(self._h)))
        cap, dev = int(cap), self.device
        out = SimpleNamespace(coords=torch.empty((n, cap, 2), dtype=torch.int16, device=dev),
                              length=torch.empty(n, dtype=torch.int32, device=dev),
                              overlay=torch.empty((n,) + self.map_shape, dtype=torch.uint8, device=dev) if overlay else None)
        ov = out.overlay.data_ptr() if overlay else None
        if grids is None:
            _lib.check(self._L.pcgrl_paths(self._h, cap, out.coords.data_ptr(), out.length.data_ptr(), ov, self._stream()),
                       "pcgrl_paths")
        else:
            _lib.check(self._L.pcgrl_paths_for_grids(self._h, n, grids.data_ptr(), cap, out.coords.data_ptr(),
                                                     out.length.data_ptr(), ov, self._stream()), "pcgrl_paths_for_grids")
        return out

    def paths(self, cap=None, overlay=False):
        """The solution path of every env's current map, as the reference keeps it for rendering (binary:
        _prob.path_coords, binary_prob.py:152-158; zelda: _prob.path with render_path, zelda_ctrl_prob.py:153-165):
          coords  int16 [N, cap, 2]  the first min(length, cap) cells as (row, col), then (-1, -1)
          length  int32 [N]          the full length (binary: path-length + 1, or 0)
          overlay uint8 [N, H, W]    1 on the path's cells (overlay=True), else None
        cap=None: the longest path the map shape allows.  A function of the map alone (stale statistics do not matter);
        one launch on the current stream, no host sync.  sokoban / the 3-D maze: NotImplementedError."""
        return self._paths(self.num_envs, None, cap, overlay)

    def paths_for_grids(self, grids, cap=None, overlay=False):
        """paths() of caller maps (any number of them, uint8 tile ids of this env's problem and map shape)."""
        g = torch.as_tensor(grids, device=self.device).to(torch.uint8).contiguous()
        return self._paths(g.numel() // self.n_cells, g, cap, overlay)

    # -- sokoban solutions (include/pcgrl_amd_solutions.h) -----------------------------------------------------------
    def _solutions(self, n, grids, cap, dist_win):
        if cap is None:  # (a problem without a solver reports 0: the call below is what refuses it)
            cap = max(1, int(self._L.pcgrl_solution_capacity(self._h)))
        cap, dev = int(cap), self.device
        out = SimpleNamespace(moves=torch.empty((n, cap), dtype=torch.int8, device=dev),
                              length=torch.empty(n, dtype=torch.int32, device=dev),
                              dist_win=torch.empty(n, dtype=torch.int32, device=dev) if dist_win else None)
        dw = out.dist_win.data_ptr() if dist_win else None
        if grids is None:
            _lib.check(self._L.pcgrl_solutions(self._h, cap, out.moves.data_ptr(), out.length.data_ptr(), dw, self._stream()),
                       "pcgrl_solutions")
        else:
            _lib.check(self._L.pcgrl_solutions_for_grids(self._h, n, grids.data_ptr(), cap, out.moves.data_ptr(),
                                                         out.length.data_ptr(), dw, self._stream()),
                       "pcgrl_solutions_for_grids")
        return out

    def solutions(self, cap=None, dist_win=False):
        """The solution of every env's current sokoban map: the move list the reference's get_stats leaves in
        stats["solution"] (sokoban_prob.py:178), whose length is `sol-length`:
          moves     int8 [N, cap]   the first min(length, cap) moves in playing order as indices into the reference's
                                    `directions` (engine.py:3: 0 = x-1, 1 = x+1, 2 = y-1, 3 = y+1), then -1
          length    int32 [N]       the full length; 0: no stage of the solver won; -1: the solver's precondition (one
                                    player, crates == targets > 0, one region) does not hold
          dist_win  int32 [N]       `dist-win` of the statistics (dist_win=True), else None
        cap=None: solver_power, the longest solution there can be.  A function of the map and solver_power alone (stale
        statistics and a solver budget do not matter); one launch on the current stream, no host sync.  Other problems:
        NotImplementedError."""
        return self._solutions(self.num_envs, None, cap, dist_win)

    def solutions_for_grids(self, grids, cap=None, dist_win=False):
        """solutions() of caller maps (any number of them, uint8 tile ids of this env's map shape)."""
        g = torch.as_tensor(grids, device=self.device).to(torch.uint8).contiguous()
        return self._solutions(g.numel() // self.n_cells, g, cap, dist_win)

    # -- level measures and pairwise Hamming diversity (include/pcgrl_amd_measures.h) ------------------------------------
    _meas_set_device = False  # (every entry point takes the handle and sets its device)

    def _meas_dims(self):
        return self.n_cells, self.spec.n_tiles

    def _measures_supported(self):
        if len(self.map_shape) != 2:  # (the entry point refuses the 3-D maze before it looks at its pointers: its reason)
            _lib.check(self._L.pcgrl_measures(self._h, None, None, None, None, None, None), "pcgrl_measures")

    def _measures(self, n, grids, entropy):
        self._measures_supported()
        if grids is None:
            return self._measures_result(self._L.pcgrl_measures, (self._h,), n, entropy)
        return self._measures_result(self._L.pcgrl_measures_for_grids, (self._h, n, grids.data_ptr()), n, entropy)

    def measures(self, entropy=True):
        """The behaviour characteristics of every env's current map that the reference computes from the integer map
        (evo/evolve.py:606-635 get_bc -> :423-592):
          counts          int32 [N, T]    cells per tile type
          match           int32 [N, 3]    horizontal matches, vertical matches, wrapped co-occurance matches
          tile_fractions  float64 [N, T]  get_counts
          bc              dict keyed by get_bc's names -> float64 [N]: "emptiness", "entropy" (entropy=True), "symmetry",
                          "symmetry-horizontal", "symmetry-vertical", "co-occurance" (also .entropy, .emptiness)
        All but entropy equal the reference bit for bit; entropy does on the host whose numpy built the table.  A function of
        the maps alone (stale statistics do not matter); one kernel launch on the current stream, no host sync.  The 3-D maze: NotImplementedError."""
        return self._measures(self.num_envs, None, entropy)

    def measures_for_grids(self, grids, entropy=True):
        """measures() of caller maps (any number of them, uint8 tile ids of this env's problem and map shape)."""
        g = torch.as_tensor(grids, device=self.device).to(torch.uint8).contiguous()
        return self._measures(g.numel() // self.n_cells, g, entropy)

    def _diversity(self, n, grids, group, pairwise):
        self._measures_supported()
        fn, head = self._L.pcgrl_diversity, (self._h,)
        if grids is not None:
            fn, head = self._L.pcgrl_diversity_for_grids, (self._h, n, grids.data_ptr())
        return self._diversity_result(fn, head, n, group, pairwise, self._L.pcgrl_diversity_scratch_bytes(self._h, n))

    def diversity(self, group=None, pairwise=False):
        """Pairwise Hamming distances (cells whose tiles differ) among the envs' current maps, in consecutive groups of `group`
        maps (None: one group of all of them):
          hamming_sum      int64 [G]      the sum over all ordered pairs of a group
          nearest          int32 [N]      the distance to the nearest other map of the group
          nearest_idx      int32 [N]      that map's index within the group, the lowest on ties
          div_score        float64 [G]    div_calc (rl/evaluate_ctrl.py:42-48)
          diversity_bonus  float64 [G]    evo/evolve.py:1236-1244 (its denominator is K * K - 1)
          pairwise         int32 [G, K, K] (pairwise=True), else None
        Three kernel launches (pack, all pairs, finish) on the current stream, no host sync.  The 3-D maze: NotImplementedError."""
        return self._diversity(self.num_envs, None, group, pairwise)

    def diversity_for_grids(self, grids, group=None, pairwise=False):
        """diversity() of caller maps (any number of them, uint8 tile ids of this env's problem and map shape)."""
        g = torch.as_tensor(grids, device=self.device).to(torch.uint8).contiguous()
        return self._diversity(g.numel() // self.n_cells, g, group, pairwise)

    # -- episodic-return reduction (rl/callbacks.py:91-117 on_episode_end, summed over the batch) -------------------
    def reduce_episodes(self, clear=True, out=None):
        """float64 [3 + n_stats] on the env's GPU: sum of returns, sum of lengths, number of episodes, sum of final
        stats over the episodes that ended by auto-reset since the last clearing call.  One launch, no sync."""
        if out is None:
            out = torch.empty(3 + self.n_stats, dtype=torch.float64, device=self.device)
        _lib.check(self._L.pcgrl_reduce_episodes(self._h, out.data_ptr(), 1 if clear else 0, self._stream()),
                   "pcgrl_reduce_episodes")
        return out

    # -- checkpoint / restore (envs/pcgrl_env.py:102-112 get_task / set_task pickle the env) ------------------------
    def get_rng_state(self):
        """uint64-as-int64 [N, 10]: both numpy-compatible PCG64 streams of every env (see include/pcgrl_amd.h)."""
        out = torch.empty((self.num_envs, 10), dtype=torch.int64, device=self.device)
        _lib.check(self._L.pcgrl_get_rng_state(self._h, out.data_ptr(), self._stream()), "pcgrl_get_rng_state")
        return out

    def set_rng_state(self, rng, mask=None):
        r = torch.as_tensor(rng, device=self.device).to(torch.int64).contiguous()
        assert r.shape == (self.num_envs, 10)
        m = None if mask is None else torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        _lib.check(self._L.pcgrl_set_rng_state(self._h, m.data_ptr() if m is not None else None, r.data_ptr(),
                                               self._stream()), "pcgrl_set_rng_state")

    def state_dict(self):
        """Everything needed to continue bit-exactly later.  `blob` is the engine's complete per-env state
        (pcgrl_export_state: maps, incremental-statistics masks, counters, statistics, returns and episode totals, RNG
        streams, static-tile masks / lagging bordered planes / spare RNG half, active and queued control targets, the 3-D
        move table and cached searches) -- what pickling the reference's env keeps (pcgrl_env.py:102-112,
        reps/wrappers.py:80-87); the portable fields (maps, positions, counters, returns, RNG streams) ride along."""
        st = self.get_state()
        blob = torch.empty(int(self._L.pcgrl_state_bytes(self._h)), dtype=torch.uint8, device=self.device)
        stale = C.c_int32(0)
        _lib.check(self._L.pcgrl_export_state(self._h, blob.data_ptr(), C.byref(stale), self._stream()), "pcgrl_export_state")
        return {"grids": st.grids.clone(), "pos": st.pos.clone(), "counters": st.counters.clone(),
                "ep_return": st.ep_return.clone(), "rng": self.get_rng_state(), "blob": blob, "maybe_stale": int(stale.value)}

    def load_state_dict(self, sd, mask=None):
        def dev(t, dtype):
            return torch.as_tensor(t, device=self.device).to(dtype).contiguous()

        m = None if mask is None else dev(mask, torch.uint8)
        if "blob" in sd:
            b = dev(sd["blob"], torch.uint8)
            if b.numel() != int(self._L.pcgrl_state_bytes(self._h)):
                raise ValueError("state_dict from an engine with another config or batch size")
            _lib.check(self._L.pcgrl_import_state(self._h, m.data_ptr() if m is not None else None, b.data_ptr(),
                                                  int(sd.get("maybe_stale", 1)), self._stream()), "pcgrl_import_state")
            return
        g, p, c = dev(sd["grids"], torch.uint8), dev(sd["pos"], torch.int32), dev(sd["counters"], torch.int32)
        r = dev(sd["ep_return"], torch.float64)
        assert g.numel() == self.num_envs * self.n_cells and p.shape == (self.num_envs, 3) and c.shape == (self.num_envs, 4)
        _lib.check(self._L.pcgrl_set_state(self._h, m.data_ptr() if m is not None else None, g.data_ptr(), p.data_ptr(),
                                           c.data_ptr(), r.data_ptr(), self._stream()), "pcgrl_set_state")
        self.set_rng_state(sd["rng"], mask=mask)


class SubBatchedVecEnv:
    """The batch cut into k independent sub-batches: k engines of N / k envs, each launched on a HIP stream of its own.

    A step launch lasts as long as its slowest env (one long path search); with k chains a launch only waits for the
    slowest env of ITS sub-batch and the chains overlap on the device (`async_sub_batches`: up to
    1.3 x on 64 x 64 maps and the 15^3 maze, a loss on the 16 x 16 maps whose launches are already short).  Envs are
    independent objects in the reference too (rl/utils.py:412-415 workers x envs); results are those of one batch of N.

      step(actions)              all k launches forked from / joined back into the current stream: drop-in for
                                 VecPcgrlEnv.step (outputs are [N, ...] tensors, sub-batch i owns rows [i*n, (i+1)*n)),
                                 also under HIP-graph capture (k parallel branches)
      step_async(i, actions_i)   launch sub-batch i alone on its stream -> its rows of the outputs; wait(i) makes the
                                 current stream wait for it (Sample-Factory-style double buffering: the policy runs on
                                 sub-batch i's observation while sub-batch j steps)
    """

    def __init__(self, problem, representation, map_shape, num_envs, sub_batches, device="cuda:0", seeds=None, **kw):
        k = int(sub_batches)
        if k < 1 or num_envs % k:
            raise ValueError("num_envs must be a multiple of sub_batches")
        self.k, self.num_envs, self.n_sub = k, int(num_envs), int(num_envs) // k
        self.device = torch.device(device)
        seeds = np.arange(num_envs) if seeds is None else np.broadcast_to(np.asarray(seeds), (num_envs,))
        n = self.n_sub
        cfg, spec, obs_window = build_config(problem, representation, map_shape, **{a: kw[a] for a in _CONFIG_ARGS if a in kw})
        obs_shape = obs_shape_for(cfg, spec, obs_window, kw.get("obs_format", "onehot"))
        N, dev = self.num_envs, self.device
        self._obs = torch.empty((N,) + obs_shape, dtype=torch.uint8, device=dev)
        self._reward = torch.empty(N, dtype=torch.float32, device=dev)
        self._done = torch.empty(N, dtype=torch.uint8, device=dev)
        self._stats = torch.empty((N, len(spec.stat_keys)), dtype=torch.int32, device=dev)
        self.streams = [torch.cuda.Stream(dev) for _ in range(k)]
        self.envs = []
        for i in range(k):
            sl = slice(i * n, (i + 1) * n)
            self.envs.append(VecPcgrlEnv(problem, representation, map_shape, n, device=dev, seeds=seeds[sl],
                                         _out=(self._obs[sl], self._reward[sl], self._done[sl], self._stats[sl]), **kw))
        e0 = self.envs[0]
        assert e0.obs_shape == obs_shape, (e0.obs_shape, obs_shape)
        for a in ("obs_shape", "num_actions", "action_entries", "stat_keys", "n_stats", "spec", "cfg", "map_shape", "auto_reset",
                  "problem", "representation", "obs_format", "onehot_shape"):
            setattr(self, a, getattr(e0, a))
        done = self._done.view(torch.bool)
        self._step_out = (self._obs, self._reward, done, done, {"stats": self._stats})

    def close(self):
        for e in self.envs:
            e.close()

    def _fork(self, i):
        self.streams[i].wait_stream(torch.cuda.current_stream(self.device))

    def wait(self, i=None):
        """the current stream waits for sub-batch i's stream (None: for all of them)"""
        cur = torch.cuda.current_stream(self.device)
        for j in (range(self.k) if i is None else (i,)):
            cur.wait_stream(self.streams[j])

    def _each(self, call):
        """[call(i, envs[i]) for every sub-batch i], each on its sub-batch's stream -- ordered after the work queued on the
        current stream and on that stream (a step_async in flight) -- then joined back into the current stream"""
        out = []
        for i, e in enumerate(self.envs):
            self._fork(i)
            with torch.cuda.stream(self.streams[i]):
                out.append(call(i, e))
        self.wait()
        return out

    def reset(self, **kw):
        self._each(lambda i, e: e.reset(**{key: self._rows(v, i) for key, v in kw.items()}))
        return self._obs, {}

    def step_async(self, i, actions):
        """sub-batch i alone, on its own stream (ordered after the work already queued on the current stream); returns
        the sub-batch's step tuple -- valid once wait(i) has been called (or its stream synchronised)"""
        self._fork(i)
        # `actions` was allocated on the caller's stream and is read on streams[i]: a temporary (policy(obs).argmax().int())
        # freed right after this call must not be handed out again before that read has happened (not while capturing:
        # a captured graph keeps its buffers alive itself)
        if isinstance(actions, torch.Tensor) and actions.is_cuda and not torch.cuda.is_current_stream_capturing():
            actions.record_stream(self.streams[i])
        with torch.cuda.stream(self.streams[i]):
            return self.envs[i].step(actions)

    def step(self, actions):
        if self.envs[0]._ex:
            raise NotImplementedError("controllable mode / float64 rewards: use step_async(i, ...) (per-sub-batch outputs)")
        n = self.n_sub
        a = actions.reshape(self.num_envs, -1)
        for i in range(self.k):
            self.step_async(i, a[i * n:(i + 1) * n])
        self.wait()
        return self._step_out

    def _cat(self, parts, keys, **rest):
        return SimpleNamespace(**{**rest, **{key: torch.cat([getattr(p, key) for p in parts]) for key in keys}})

    def get_state(self):
        return self._cat(self._each(lambda i, e: e.get_state()),
                         ("grids", "pos", "counters", "stats", "last_loss", "ep_return", "iteration", "changes", "n_step", "ep_len"))

    def paths(self, cap=None, overlay=False):
        return self._cat(self._each(lambda i, e: e.paths(cap=cap, overlay=overlay)),
                         ("coords", "length") + (("overlay",) if overlay else ()), overlay=None)

    def solutions(self, cap=None, dist_win=False):
        return self._cat(self._each(lambda i, e: e.solutions(cap=cap, dist_win=dist_win)),
                         ("moves", "length") + (("dist_win",) if dist_win else ()), dist_win=None)

    def measures(self, entropy=True):
        parts = self._each(lambda i, e: e.measures(entropy=entropy))
        out = self._cat(parts, ("counts", "match", "forms") + (("entropy",) if entropy else ()), entropy=None)
        f = out.forms
        out.tile_fractions = f[:, 5:]
        out.bc = {"emptiness": f[:, 0], "symmetry-horizontal": f[:, 1], "symmetry-vertical": f[:, 2], "symmetry": f[:, 3],
                  "co-occurance": f[:, 4]}
        if entropy:
            out.bc["entropy"] = out.entropy
        out.emptiness = out.bc["emptiness"]
        return out

    def diversity(self, group=None, pairwise=False):
        raise NotImplementedError("diversity over sub-batches: a group could straddle two engines -- gather the maps "
                                  "(get_state().grids) and call envs[0].diversity_for_grids(grids, group)")

    def reduce_episodes(self, clear=True):
        return torch.stack(self._each(lambda i, e: e.reduce_episodes(clear=clear))).sum(0)

    def last_episode(self):
        return self._cat(self._each(lambda i, e: e.last_episode()), ("ep_return", "ep_len", "final_stats", "n_episodes"))

    def sample_actions(self, seed=0):
        """one device-side draw per sub-batch (sub-batch i uses seed + i: its engines keep their own draw counters)"""
        return torch.cat(self._each(lambda i, e: e.sample_actions(seed + i)))

    def observe(self):
        self._each(lambda i, e: e.observe())
        return self._obs

    def state_dict(self):
        """a list of the sub-batches' checkpoints (VecPcgrlEnv.state_dict); loads into an env with the same split"""
        return {"sub_batches": self._each(lambda i, e: e.state_dict())}

    def load_state_dict(self, sd, mask=None):
        if len(sd.get("sub_batches", ())) != self.k:
            raise ValueError(f"state_dict of {len(sd.get('sub_batches', ()))} sub-batches, this env has {self.k}")
        self._each(lambda i, e: e.load_state_dict(sd["sub_batches"][i], mask=self._rows(mask, i)))

    def check_errors(self):
        for e in self.envs:
            e.check_errors()

    # -- the rest of VecPcgrlEnv's surface, fanned out over the sub-batches ---------------------------------------------
    def _rows(self, v, i):
        """sub-batch i's rows of a per-env value; None, scalars (0-dim tensors too) and (lo, hi) target tuples are the same
        for every sub-batch"""
        if v is None or isinstance(v, tuple) or np.ndim(v) == 0:
            return v
        return (v if hasattr(v, "shape") else torch.as_tensor(v))[i * self.n_sub:(i + 1) * self.n_sub]

    def seed(self, seeds):
        s = np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (self.num_envs,))
        self._each(lambda i, e: e.seed(self._rows(s, i)))

    def set_static(self, static_prob=None, n_static_walls=None, eval_mode=None):
        for e in self.envs:  # (engine parameters on the host, read by the next reset)
            e.set_static(static_prob, n_static_walls, eval_mode)

    def get_static(self):
        return torch.cat(self._each(lambda i, e: e.get_static()))

    def queue_targets(self, trgs, mask=None):
        self._each(lambda i, e: e.queue_targets({k: self._rows(v, i) for k, v in trgs.items()}, mask=self._rows(mask, i)))

    def set_target_resampling(self, enable=True, seed=0):
        raise NotImplementedError("target resampling draws from (seed, env index): per sub-batch the env indices restart at 0 -- use one "
                                  "VecPcgrlEnv, or call envs[i].set_target_resampling with distinct seeds")

    @property
    def ctrl_obs(self):
        self.wait()
        return None if self.envs[0].ctrl_obs is None else torch.cat([e.ctrl_obs for e in self.envs])

    def get_rng_state(self):
        return torch.cat(self._each(lambda i, e: e.get_rng_state()))

    def set_rng_state(self, rng, mask=None):
        self._each(lambda i, e: e.set_rng_state(self._rows(rng, i), mask=self._rows(mask, i)))

    def solver_pool_slots(self):
        """(slots, full size, failed) summed over the sub-batches' engines (each keeps a pool of its own)"""
        parts = [e.solver_pool_slots() for e in self.envs]
        return sum(p[0] for p in parts), sum(p[1] for p in parts), any(p[2] for p in parts)

    def rollout(self, actions, want_obs="all"):
        raise NotImplementedError("open-loop rollouts: use VecPcgrlEnv (a rollout's waves advance independently already)")


def make_vec_env(cfg, num_envs, device="cuda:0", seeds=None, auto_reset=True, sub_batches=1):
    """Batched counterpart of control_pcgrl/rl/envs.py:make_env(cfg).  `cfg` is the reference's Config-like
    object (attributes or dict keys): task.problem, task.map_shape, task.obs_window, task.weights,
    representation, max_board_scans, change_percentage; obs_format ("onehot" default, or "codes": VecPcgrlEnv).
    cfg.multiagent.n_agents != 0 (with or without cfg.show_agents): a multiagent.MultiAgentVecEnv.
    cfg.task.problem == "smb" (narrow, turtle): a smb_env.SmbVecEnv."""
    if _cfg_get(cfg, "task.problem") == "smb":  # an env class of its own: the engine does not know the problem
        from .smb_env import make_smb_vec_env
        return make_smb_vec_env(cfg, num_envs, device=device, seeds=seeds, auto_reset=auto_reset, sub_batches=sub_batches)
    unsupported = {
        "n_aux_tiles": _cfg_get(cfg, "n_aux_tiles", 0) or None,
    }
    bad = {k: v for k, v in unsupported.items() if v not in (None, 0, False)}
    if bad:
        raise NotImplementedError(f"outside the accelerated hot path (SURVEY.md section 8f 'next'): {bad}")
    if _cfg_get(cfg, "multiagent.n_agents", 0):
        from .multiagent import make_multiagent_vec_env
        return make_multiagent_vec_env(cfg, num_envs, device=device, seeds=seeds, auto_reset=auto_reset, sub_batches=sub_batches)
    if _cfg_get(cfg, "show_agents", False):
        raise NotImplementedError("show_agents needs multiagent.n_agents >= 2 (the reference's ShowAgentRepresentation has no "
                                  "positions to show without the multi-agent wrapper)")
    if int(sub_batches) > 1 and _cfg_get(cfg, "controls"):
        raise NotImplementedError("sub_batches > 1 with cfg.controls: SubBatchedVecEnv.step() has no float64 rewards / control "
                                  "observation of the whole batch (use sub_batches=1, or step_async per sub-batch)")
    ctor = VecPcgrlEnv if int(sub_batches) <= 1 else (lambda **kw: SubBatchedVecEnv(sub_batches=sub_batches, **kw))
    return ctor(
        problem=_cfg_get(cfg, "task.problem"), representation=_cfg_get(cfg, "representation"),
        map_shape=tuple(_cfg_get(cfg, "task.map_shape")), num_envs=num_envs, device=device,
        obs_window=_cfg_get(cfg, "task.obs_window"), weights=_cfg_get(cfg, "task.weights"),
        max_board_scans=_cfg_get(cfg, "max_board_scans", 3), change_percentage=_cfg_get(cfg, "change_percentage"),
        seeds=seeds, auto_reset=auto_reset, controls=_cfg_get(cfg, "controls"),
        reward_dtype=torch.float64 if _cfg_get(cfg, "controls") else torch.float32,
        act_window=_cfg_get(cfg, "act_window"), static_prob=_cfg_get(cfg, "static_prob"),
        n_static_walls=_cfg_get(cfg, "n_static_walls"), obs_format=_cfg_get(cfg, "obs_format", "onehot") or "onehot")
