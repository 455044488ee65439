"""Stepping Super Mario Bros environments on the device: what make_env(cfg) of the reference does for smb with the narrow or
the turtle representation -- reset, update, the nine statistics, reward, done, the cropped one-hot observation and the automatic
reset -- for a batch of envs, one launch per step (include/pcgrl_amd_smb_env.h, csrc/smb/pcgrl_smb_env.h).

SMB does not fit the 2-D engine (a map up to 128 columns of bytes, nine statistics), so this is an env class of its own next to
the evaluator of smb.py: PROBLEMS / problem_spec / build_config still do not know "smb", and make_vec_env / make_env dispatch
here on cfg.task.problem == "smb".  file:line references are relative to the reference's control_pcgrl/ directory.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .problems import target_interval
from .smb import MAX_H, MAX_SOLVER_POWER, MAX_W, MIN_H, SMB_TILES, SmbMeasures, smb_config, smb_spec

REPS = {"narrow": 0, "turtle": 1}
MAX_OBS_WINDOW = 255  # Cropped.set_pad_size keeps the pad as int8: the reference fails above


_OBS_MODES = {"none": 0, "last": 1, "all": 2}  # obs_mode of include/pcgrl_amd_smb_rollout.h
_MASK64 = (1 << 64) - 1


def sampled_actions(seed, first_draw, n_steps, num_envs, num_actions):
    """The device-drawn actions on the host: int32 [n_steps, num_envs], row k the draw first_draw + k under `seed` -- what
    SmbVecEnv.sample_actions and rollout(n_steps=...) take (include/pcgrl_amd_smb_rollout.h has the function)."""
    def mix64(z):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return z ^ (z >> np.uint64(31))

    with np.errstate(over="ignore"):
        c = np.uint64(int(first_draw) & _MASK64) + np.arange(int(n_steps), dtype=np.uint64)
        a = mix64(np.uint64(int(seed) & _MASK64) + c * np.uint64(0x9e3779b97f4a7c15))
        i = np.arange(int(num_envs), dtype=np.uint64) * np.uint64(0xd1b54a32d192ed03) + np.uint64(0x8cb92ba72f3d8dd7)
        r = mix64(a[:, None] ^ i[None, :])
    # floor(r * num_actions / 2^64) from the two 32-bit halves: num_actions < 2^31, so nothing overflows
    n = np.uint64(int(num_actions))
    hi, lo = r >> np.uint64(32), r & np.uint64(0xFFFFFFFF)
    return ((hi * n + ((lo * n) >> np.uint64(32))) >> np.uint64(32)).astype(np.int32)


def _refuse(what, why):
    raise NotImplementedError(f"smb: {what} is not stepped on the device: {why}")


class SmbVecEnv(SmbMeasures):
    """N Mario envs on one device with VecPcgrlEnv's conventions: torch tensors in and out, one HIP launch per step(), output
    tensors owned by the env and overwritten by the next call.  There is no CPU fallback.

    step(actions) -> (obs uint8 [N][oh][ow][8], reward [N], done bool [N], truncated (= done), info); info["stats"] is int32
    [N][9] (stat_keys order): the statistics after the step, of the finished episode where the step ended one.  With auto_reset a
    finished env draws its next episode inside the same launch and the observation returned is that episode's first.

    controls=[...] (statistics' names) makes the env controllable (include/pcgrl_amd_smb_ctrl.h): per-env
    targets on the device, queue_targets / set_target_resampling, info["ctrl_obs"] float32 [N][2K] = per control (target / range,
    statistic / range) from reset / step / step_ready, and float64 rewards."""

    def __init__(self, representation, map_shape=(16, 116), num_envs=1, device="cuda:0", obs_window=None, weights=None,
                 max_board_scans=3, change_percentage=None, seeds=None, auto_reset=True, solver_power=10000,
                 reward_dtype=torch.float32, controls=None):
        self._h = None
        self._L = _lib.lib()
        if representation == "wide":
            _refuse("the wide representation", "the reference's wide fails on a non-square map (wide_rep.py:42, IndexError)")
        if representation not in REPS:
            raise ValueError(f"unknown representation {representation!r}")
        map_shape = tuple(int(s) for s in map_shape)
        if len(map_shape) != 2:
            raise ValueError(f"smb maps are 2-D, got shape {map_shape}")
        H, W = map_shape
        if not (MIN_H <= H <= MAX_H and 1 <= W <= MAX_W) or not 1 <= int(solver_power) <= MAX_SOLVER_POWER:
            raise NotImplementedError(f"smb: map_shape {map_shape} / solver_power {solver_power} outside {MIN_H}..{MAX_H} x "
                                      f"1..{MAX_W} and 1..{MAX_SOLVER_POWER}")
        obs_window = (2 * H, 2 * W) if obs_window is None else tuple(int(s) for s in obs_window)  # rl/utils.py:302-334
        if len(obs_window) != 2 or min(obs_window) < 1:
            raise ValueError(f"obs_window must be two positive sizes, got {obs_window}")
        if max(obs_window) > MAX_OBS_WINDOW:
            _refuse(f"obs_window {obs_window}", f"an entry above {MAX_OBS_WINDOW} fails in the reference (Cropped keeps the pad as "
                    "int8: 'index can't contain negative values')")
        if reward_dtype not in (torch.float32, torch.float64):
            raise ValueError("reward_dtype must be torch.float32 or torch.float64")
        if int(num_envs) < 1:
            raise ValueError("num_envs must be at least 1")
        self.representation, self.map_shape, self.obs_window = representation, map_shape, obs_window
        self.num_envs, self.auto_reset, self.solver_power = int(num_envs), bool(auto_reset), int(solver_power)
        self.spec = smb_spec(map_shape)
        self.stat_keys = list(self.spec.stat_keys)
        self.controls = list(controls) if controls else []
        for k in self.controls:
            if k not in self.stat_keys:
                raise ValueError(f"'{k}' is not an smb statistic ({self.stat_keys})")
        if len(set(self.controls)) != len(self.controls):
            raise ValueError(f"a control metric is listed twice: {self.controls}")
        if self.controls:
            reward_dtype = torch.float64  # as make_vec_env: float targets make rewards that float32 would round
        self.num_actions = len(SMB_TILES) if representation == "narrow" else 4 + len(SMB_TILES)
        self.obs_shape = obs_window + (len(SMB_TILES) + 1,)
        self.max_iterations = H * W * int(max_board_scans) + 1  # pcgrl_env.py:241
        self.max_changes = None if change_percentage is None else max(int(change_percentage * H * W), 1)  # :235-239
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("SmbVecEnv needs a cuda device: there is no CPU fallback")
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        base = smb_config(map_shape, solver_power, weights)
        cfg = _lib.PcgrlSmbEnvConfig()
        cfg.h, cfg.w, cfg.representation = H, W, REPS[representation]
        cfg.obs_window[0], cfg.obs_window[1] = obs_window
        cfg.max_iterations = self.max_iterations
        cfg.max_changes = -1 if self.max_changes is None else self.max_changes
        cfg.solver_power, cfg.n_envs = self.solver_power, self.num_envs
        for i in range(9):
            cfg.has_trg[i], cfg.weight[i], cfg.trg_lo[i], cfg.trg_hi[i] = base.has_trg[i], base.weight[i], base.trg_lo[i], base.trg_hi[i]
        self.cfg = cfg
        self.weights = {k: float(cfg.weight[i]) for i, k in enumerate(self.stat_keys)}
        nbytes = self._L.pcgrl_smb_env_workspace_bytes(C.byref(cfg))
        if nbytes < 0:
            raise NotImplementedError("smb: " + self._L.pcgrl_last_error().decode())
        N, dev = self.num_envs, self.device
        self._workspace = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        h = C.c_void_p()
        _lib.check(self._L.pcgrl_smb_env_create(C.byref(cfg), self._dev_index, self._workspace.data_ptr(), nbytes, C.byref(h)),
                   "pcgrl_smb_env_create")
        self._h = h
        self._obs = torch.empty((N,) + self.obs_shape, dtype=torch.uint8, device=dev)
        self._reward = torch.empty(N, dtype=reward_dtype, device=dev)
        self._done = torch.empty(N, dtype=torch.bool, device=dev)
        self._stats = torch.empty((N, 9), dtype=torch.int32, device=dev)
        self._r32 = self._reward.data_ptr() if reward_dtype == torch.float32 else None
        self._r64 = self._reward.data_ptr() if reward_dtype == torch.float64 else None
        self._step_out = (self._obs, self._reward, self._done, self._done, {"stats": self._stats})
        self._ctrl_obs, self._reset_info = None, {}
        if self.controls:
            K = len(self.controls)
            idx = np.array([self.stat_keys.index(k) for k in self.controls], dtype=np.int32)
            self.ctrl_ranges = {k: abs(self.spec.cond_bounds[k][1] - self.spec.cond_bounds[k][0]) for k in self.controls}
            rng = np.array([self.ctrl_ranges[k] for k in self.controls], dtype=np.float64)
            shown = np.array([self._shown(self.spec.static_trgs[k]) for k in self.controls], dtype=np.float64)
            self._ctrl_obs = torch.zeros((N, 2 * K), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(self._L.pcgrl_smb_ctrl_attach(h, K, idx.ctypes.data, rng.ctypes.data, shown.ctypes.data,
                                                         self._ctrl_obs.data_ptr()), "pcgrl_smb_ctrl_attach")
            self._reset_info = {"ctrl_obs": self._ctrl_obs}
            self._step_out[4]["ctrl_obs"] = self._ctrl_obs
        if seeds is not None:
            self.seed(seeds)

    def _stream(self):
        try:
            return torch._C._cuda_getCurrentRawStream(self._dev_index)
        except AttributeError:  # pragma: no cover
            return torch.cuda.current_stream(self.device).cuda_stream

    def _handle(self):
        if self._h is None:
            raise RuntimeError("SmbVecEnv is closed")
        return self._h

    def seed(self, seeds):
        """Env i gets numpy PCG64(SeedSequence(seeds[i])) for both RNG streams (envs/pcgrl_env.py:142-146)."""
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (self.num_envs,)))
        _lib.check(self._L.pcgrl_smb_env_seed(self._handle(), s.ctypes.data), "pcgrl_smb_env_seed")

    def reset(self, mask=None, init_grids=None, init_pos=None):
        """Resets the envs of `mask` (all without one).  init_grids uint8 [N][H][W] replaces the drawn maps and draws nothing from
        the streams, as VecPcgrlEnv.reset does; init_pos [N][2] is the turtle's start on them (narrow starts at cell 0)."""
        def dev(t, dtype, shape):
            if t is None:
                return None
            t = torch.as_tensor(t, device=self.device).to(dtype).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"expected shape {list(shape)}, got {list(t.shape)}")
            return t

        N = self.num_envs
        m = dev(mask, torch.uint8, (N,))
        g = dev(init_grids, torch.uint8, (N,) + self.map_shape)
        p = dev(init_pos, torch.int32, (N, 2))
        if p is not None and g is None:
            raise ValueError("init_pos needs init_grids")
        with torch.cuda.device(self.device):
            _lib.check(self._L.pcgrl_smb_env_reset(self._handle(), m.data_ptr() if m is not None else None,
                                                   g.data_ptr() if g is not None else None,
                                                   p.data_ptr() if p is not None else None, self._obs.data_ptr(), self._stream()),
                       "pcgrl_smb_env_reset")
        return self._obs, self._reset_info

    # -- controllable generation (control_wrappers.py:27-121; include/pcgrl_amd_smb_ctrl.h) -------------------------------------
    @property
    def ctrl_obs(self):
        """float32 [N][2K], written by the last reset / step / step_ready / rollout / set_state (None without controls)"""
        return self._ctrl_obs

    @staticmethod
    def _shown(trg):
        # control_wrappers.py:203-204: a tuple target shows the midpoint of the raw tuple, not of its zero-loss interval
        return (trg[0] + trg[1]) / 2 if isinstance(trg, tuple) else float(trg)

    def _need_controls(self):
        if not self.controls:
            raise ValueError("this env was built without `controls`")

    def queue_targets(self, trgs, mask=None):
        """ControlWrapper.set_trgs: `trgs` = {metric: scalar | (lo, hi) | tensor [N]}; the targets take effect at each env's
        next reset (explicit or automatic) and replace those of the named metrics only; a second call before that reset
        replaces the first (control_wrappers.py:167-178).  A tuple means the reference's min |arange(lo, hi) - value|, so its
        lo must be a whole number (the statistics are integers; hi need not be)."""
        self._need_controls()
        if not trgs:
            raise ValueError("queue_targets needs at least one metric")
        N, dev = self.num_envs, self.device
        named, cols = [], []
        for k, v in trgs.items():
            if k not in self.controls:
                raise ValueError(f"'{k}' is not a control metric of this env ({self.controls})")
            named.append(self.controls.index(k))
            if isinstance(v, tuple):
                if len(v) != 2 or float(v[0]) != int(v[0]):
                    raise ValueError(f"a tuple target is (lo, hi) with a whole-number lo, got {v!r}")
                a, b = target_interval((float(v[0]), float(v[1])))
                lo, hi, sh = (torch.full((N,), x, dtype=torch.float64, device=dev) for x in (a, b, self._shown(v)))
            else:
                t = torch.as_tensor(v, dtype=torch.float64, device=dev)
                if t.dim() > 1 or (t.dim() == 1 and t.numel() != N):
                    raise ValueError(f"a tensor target must be [{N}], got {tuple(t.shape)}")
                lo = hi = sh = t.expand(N) if t.dim() == 0 else t
            cols.append((lo, hi, sh))
        lo, hi, sh = (torch.stack([c[i] for c in cols], dim=1).contiguous() for i in range(3))
        m = None if mask is None else self._dev(mask, torch.uint8, (N,))
        nm = np.array(named, dtype=np.int32)
        _lib.check(self._L.pcgrl_smb_ctrl_queue(self._handle(), self._ptr(m), len(named), nm.ctypes.data, lo.data_ptr(),
                                                hi.data_ptr(), sh.data_ptr(), self._stream()), "pcgrl_smb_ctrl_queue")

    def sample_uniform_targets(self, generator=None, mask=None):
        """UniformNoiseyTargets.set_rand_trgs (control_wrappers.py:453-460): each control target ~ U(cond_bounds), queued."""
        self._need_controls()
        trgs = {}
        for k in self.controls:
            lb, ub = self.spec.cond_bounds[k]
            u = torch.rand(self.num_envs, generator=generator, device=self.device, dtype=torch.float64)
            trgs[k] = u * (ub - lb) + lb
        self.queue_targets(trgs, mask=mask)
        return trgs

    def set_target_resampling(self, enable=True, seed=0):
        """UniformNoiseyTargets on the device: from each env's next reset on -- explicit or automatic, also inside a captured
        HIP graph -- every control target is drawn ~ U(cond_bounds) from the env's own counter-based stream and replaces whatever
        was queued.  The draw is the engine's trg_resampled (csrc/pcgrl_kernels2d.h) with the env's draw counter."""
        self._need_controls()
        lo = np.array([self.spec.cond_bounds[k][0] for k in self.controls], dtype=np.float64)
        hi = np.array([self.spec.cond_bounds[k][1] for k in self.controls], dtype=np.float64)
        _lib.check(self._L.pcgrl_smb_ctrl_set_resampling(self._handle(), 1 if enable else 0, int(seed) & _MASK64, lo.ctypes.data,
                                                         hi.ctypes.data, self._stream()), "pcgrl_smb_ctrl_set_resampling")

    def get_targets(self):
        """The per-env control records: lo, hi float64 [N][9] (the active zero-loss intervals, stat_keys order), shown float64
        [N][K] (the value the control observation shows per control), queued float64 [N][K][3] = lo, hi, shown, queued_set
        int32 [N] (bit j: the queue names control j), pending bool [N], draws int32 [N] (the env's draw counter)."""
        self._need_controls()
        N, dev, K = self.num_envs, self.device, len(self.controls)
        active = torch.empty((N, 9, 2), dtype=torch.float64, device=dev)
        shown = torch.empty((N, 9), dtype=torch.float64, device=dev)
        queued = torch.empty((N, 9, 3), dtype=torch.float64, device=dev)
        flags = torch.empty((N, 2), dtype=torch.int32, device=dev)
        _lib.check(self._L.pcgrl_smb_ctrl_get(self._handle(), active.data_ptr(), shown.data_ptr(), queued.data_ptr(),
                                              flags.data_ptr(), self._stream()), "pcgrl_smb_ctrl_get")
        return SimpleNamespace(lo=active[:, :, 0], hi=active[:, :, 1], shown=shown[:, :K], queued=queued[:, :K],
                               queued_set=flags[:, 1], pending=(flags[:, 0] & 1) != 0, draws=flags[:, 0] >> 1)

    def observe_controls(self):
        """the control observation of the committed state, into ctrl_obs"""
        self._need_controls()
        _lib.check(self._L.pcgrl_smb_ctrl_observe(self._handle(), None, self._stream()), "pcgrl_smb_ctrl_observe")
        return self._ctrl_obs

    def step(self, actions):
        if actions.numel() != self.num_envs:
            raise ValueError(f"actions must be [{self.num_envs}], got {tuple(actions.shape)}")
        if actions.dtype != torch.int32 or not actions.is_contiguous() or actions.device != self.device:
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        rc = self._L.pcgrl_smb_env_step(self._handle(), actions.data_ptr(), 1 if self.auto_reset else 0, self._obs.data_ptr(),
                                        self._r32, self._r64, self._done.data_ptr(), self._stats.data_ptr(), self._stream())
        if rc:
            _lib.check(rc, "pcgrl_smb_env_step")
        return self._step_out

    def sample_actions(self, seed=0, out=None):
        """action_space.sample() for every env, drawn on the device: int32 [N], entry i of the handle's draw c under `seed` is
        sampled_actions(seed, c, 1, N, num_actions)[0, i].  The draw counter lives on the device and advances by 1 in stream
        order, so a captured call draws fresh actions at every replay."""
        if out is None:
            out = self.__dict__.get("_sampled")
            if out is None:
                out = self._sampled = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        elif (out.dtype != torch.int32 or out.device != self.device or not out.is_contiguous()
              or out.numel() != self.num_envs):
            raise ValueError(f"out must be a contiguous int32 tensor of {self.num_envs} entries on {self.device}")
        rc = self._L.pcgrl_smb_env_sample_actions(self._handle(), out.data_ptr(), int(seed) & _MASK64, self._stream())
        if rc:
            _lib.check(rc, "pcgrl_smb_env_sample_actions")
        return out

    def rollout(self, actions=None, n_steps=None, want_obs="last", seed=0):
        """K steps of every env in ONE launch (include/pcgrl_amd_smb_rollout.h): bit for bit what K step()
        calls give, but a launch lasts as long as its slowest env's own K steps instead of K times the batch's longest search.
        For actions that do not depend on the observations.

        actions int32 [K, N] (tensor, array or list), or None with n_steps=K: drawn on the device, the same actions as K times
        [sample_actions(seed) -> step].  want_obs: "last" -> obs [N, ...] after the last step, "all" -> [K, N, ...] (row k what
        step k would have returned), "none" -> None.  Returns a namespace: reward [K, N] (reward_dtype), done and truncated bool
        [K, N], stats int32 [K, N, 9], obs, ctrl_obs (with controls: float32 [N, 2K] after the last step, else None), actions
        int32 [K, N] (the actions taken) and episodes -- count int32 [N],
        return_sum float64 [N], length_sum int64 [N], stats_sum int64 [N, 9] over the episodes finished inside this launch.
        The tensors are owned by the env, cached per (K, want_obs) and overwritten by the next call of that form; a second
        call of a form allocates nothing and can be captured with torch.cuda.graph.  Honours auto_reset."""
        if want_obs not in _OBS_MODES:
            raise ValueError(f"want_obs must be one of {sorted(_OBS_MODES)}, got {want_obs!r}")
        N = self.num_envs
        if actions is None:
            if n_steps is None:
                raise ValueError("rollout needs actions [K, N], or n_steps for actions drawn on the device")
            K, a_ptr = int(n_steps), None
        else:
            if not isinstance(actions, torch.Tensor):
                actions = torch.as_tensor(np.asarray(actions))
            if actions.dim() != 2 or actions.shape[1] != N:
                raise ValueError(f"actions must be [K, {N}], got {tuple(actions.shape)}")
            if n_steps is not None and int(n_steps) != actions.shape[0]:
                raise ValueError(f"n_steps={n_steps} does not match actions of {actions.shape[0]} steps")
            if actions.dtype != torch.int32 or not actions.is_contiguous() or actions.device != self.device:
                actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
            K, a_ptr = int(actions.shape[0]), actions.data_ptr()
        if K < 1:
            raise ValueError(f"a rollout takes at least one step, got {K}")
        bufs = self.__dict__.setdefault("_rollouts", {})
        b = bufs.get((K, want_obs))
        if b is None:
            dev = self.device
            obs = {"none": None, "last": self._obs}[want_obs] if want_obs != "all" else torch.empty(
                (K, N) + self.obs_shape, dtype=torch.uint8, device=dev)
            done = torch.empty((K, N), dtype=torch.bool, device=dev)
            b = SimpleNamespace(
                reward=torch.empty((K, N), dtype=self._reward.dtype, device=dev), done=done, truncated=done,
                stats=torch.empty((K, N, 9), dtype=torch.int32, device=dev), obs=obs, ctrl_obs=self._ctrl_obs,
                actions=torch.empty((K, N), dtype=torch.int32, device=dev),
                episodes=SimpleNamespace(count=torch.empty(N, dtype=torch.int32, device=dev),
                                         return_sum=torch.empty(N, dtype=torch.float64, device=dev),
                                         length_sum=torch.empty(N, dtype=torch.int64, device=dev),
                                         stats_sum=torch.empty((N, 9), dtype=torch.int64, device=dev)))
            bufs[(K, want_obs)] = b
        r = b.reward.data_ptr()
        ep = b.episodes
        rc = self._L.pcgrl_smb_env_rollout(
            self._handle(), a_ptr, int(seed) & _MASK64, K, 1 if self.auto_reset else 0,
            b.obs.data_ptr() if b.obs is not None else None, _OBS_MODES[want_obs], r if self._r32 is not None else None,
            r if self._r64 is not None else None, b.done.data_ptr(), b.stats.data_ptr(), b.actions.data_ptr(),
            ep.count.data_ptr(), ep.return_sum.data_ptr(), ep.length_sum.data_ptr(), ep.stats_sum.data_ptr(), self._stream())
        if rc:
            _lib.check(rc, "pcgrl_smb_env_rollout")
        return b

    def observe(self):
        _lib.check(self._L.pcgrl_smb_env_observe(self._handle(), self._obs.data_ptr(), self._stream()), "pcgrl_smb_env_observe")
        return self._obs

    # -- the pointer-level surface an adapter drives (smb_rllib.SmbVectorEnv): caller-given device or host-mapped pinned buffers,
    #    one launch per call on `stream`, the status code returned (VecPcgrlEnv has the same names for the engine's problems) -----
    def step_into(self, actions_ptr, obs_ptr, reward_ptr, reward64_ptr, done_ptr, stats_ptr, stream):
        """pcgrl_smb_env_step: any output may be None; obs_ptr is the uint8 observation (16-byte aligned)"""
        return self._L.pcgrl_smb_env_step(self._handle(), actions_ptr, 1 if self.auto_reset else 0, obs_ptr, reward_ptr,
                                          reward64_ptr, done_ptr, stats_ptr, stream)

    def observe_into(self, obs_ptr, stream):
        """the uint8 observation of the committed state"""
        return self._L.pcgrl_smb_env_observe(self._handle(), obs_ptr, stream)

    @property
    def obs_f32_shape(self):
        """one env's float32 image: [oh][ow][2K + 8], the control planes in front"""
        return self.obs_window + (2 * len(self.controls) + len(SMB_TILES) + 1,)

    def observe_f32_into(self, ptr, stream):
        """The float32 image of the committed state, float32 [N] + obs_f32_shape, written once by a kernel of its own
        (include/pcgrl_amd_smb_vector.h); after a reset / step on the same stream.  ptr: 8-byte aligned."""
        return self._L.pcgrl_smb_env_observe_f32(self._handle(), ptr, stream)

    def reset_masked(self, mask_ptr, stream, obs_ptr=None):
        """pcgrl_smb_env_reset of the envs of the uint8 mask (None = all), drawn maps; obs_ptr None writes no observation"""
        with torch.cuda.device(self.device):
            return self._L.pcgrl_smb_env_reset(self._handle(), mask_ptr, None, None, obs_ptr, stream)

    def stats_into(self, ptr, stream):
        """the committed statistics, int32 [N][9]"""
        return self._L.pcgrl_smb_env_get_state(self._handle(), None, None, None, ptr, None, None, None, stream)

    def get_state(self):
        """grids uint8 [N][H][W], pos int32 [N][2], iteration, changes, n_step (narrow's scan counter), searches (play-throughs
        run since the env was made), stats int32 [N][9], last_loss, ep_return float64 [N], search_iterations int64 [N] and
        max_search_iterations (the most one call spent on the env)."""
        N, dev = self.num_envs, self.device
        grids = torch.empty((N,) + self.map_shape, dtype=torch.uint8, device=dev)
        pos = torch.empty((N, 2), dtype=torch.int32, device=dev)
        counters = torch.empty((N, 4), dtype=torch.int32, device=dev)
        stats = torch.empty((N, 9), dtype=torch.int32, device=dev)
        last_loss = torch.empty(N, dtype=torch.float64, device=dev)
        ep_return = torch.empty(N, dtype=torch.float64, device=dev)
        iters = torch.empty((N, 2), dtype=torch.int64, device=dev)
        _lib.check(self._L.pcgrl_smb_env_get_state(self._handle(), grids.data_ptr(), pos.data_ptr(), counters.data_ptr(),
                                                   stats.data_ptr(), last_loss.data_ptr(), ep_return.data_ptr(), iters.data_ptr(),
                                                   self._stream()), "pcgrl_smb_env_get_state")
        return SimpleNamespace(grids=grids, pos=pos, iteration=counters[:, 0], changes=counters[:, 1], n_step=counters[:, 2],
                               searches=counters[:, 3], stats=stats, last_loss=last_loss, ep_return=ep_return,
                               search_iterations=iters[:, 0], max_search_iterations=iters[:, 1])

    # -- level measures and pairwise Hamming diversity (include/pcgrl_amd_smb_measures.h) ----------------
    def measures(self, entropy=True):
        """The behaviour characteristics of every env's committed map (evo/evolve.py:606-635 get_bc), field for field
        VecPcgrlEnv.measures with T = 7; read from the handle's maps, no copy.  Under a solver budget a busy env's step in
        flight is not shown, as in get_state().  One launch on the current stream, no host sync."""
        return self._measures(self._handle(), self.num_envs, None, entropy)

    def measures_for_grids(self, grids, entropy=True):
        """measures() of caller maps (any number of them, uint8 tile ids of this env's map shape)."""
        g = self._grids_arg(grids)
        return self._measures(None, g.shape[0], g, entropy)

    def diversity(self, group=None, pairwise=False):
        """Pairwise Hamming distances among the envs' committed maps in consecutive groups of `group` maps (None: one group of
        all), field for field VecPcgrlEnv.diversity.  Three launches on the current stream, no host sync."""
        return self._diversity(self._handle(), self.num_envs, None, group, pairwise)

    def diversity_for_grids(self, grids, group=None, pairwise=False):
        """diversity() of caller maps (any number of them, uint8 tile ids of this env's map shape)."""
        g = self._grids_arg(grids)
        return self._diversity(None, g.shape[0], g, group, pairwise)

    def last_episode(self):
        """The last finished episode of every env: ep_return float64 [N], length int32 [N], stats int32 [N][9], count int32 [N]
        (how many episodes the env has finished; the other rows mean nothing while it is 0)."""
        N, dev = self.num_envs, self.device
        ret = torch.empty(N, dtype=torch.float64, device=dev)
        length = torch.empty(N, dtype=torch.int32, device=dev)
        stats = torch.empty((N, 9), dtype=torch.int32, device=dev)
        count = torch.empty(N, dtype=torch.int32, device=dev)
        _lib.check(self._L.pcgrl_smb_env_get_last_episode(self._handle(), ret.data_ptr(), length.data_ptr(), stats.data_ptr(),
                                                          count.data_ptr(), self._stream()), "pcgrl_smb_env_get_last_episode")
        return SimpleNamespace(ep_return=ret, length=length, stats=stats, count=count)

    # -- checkpoint / restore (include/pcgrl_amd_smb_state.h; envs/pcgrl_env.py:102-112 pickles the env) ----
    def _dev(self, t, dtype, shape=None):
        if t is None:
            return None
        t = torch.as_tensor(t, device=self.device).to(dtype).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {list(shape)}, got {list(t.shape)}")
        return t

    @staticmethod
    def _ptr(t):
        return t.data_ptr() if t is not None else None

    @property
    def state_bytes(self):
        """bytes of export_state()'s image"""
        return int(self._L.pcgrl_smb_state_bytes(self._handle()))

    def export_state(self, out=None):
        """uint8 [state_bytes]: the whole per-env state -- maps, records, both RNG streams, and under a solver budget each env's
        mode and pending action (a parked search itself is not carried: it starts over after an import), and with controls
        each env's control record (active and queued targets, draw counter; not the resampling switch).  One launch, no sync,
        capturable: a captured export writes `out` anew at every replay."""
        if out is None:
            # with controls the records start at the next multiple of 16: up to 15 bytes before them that the kernel does not
            # write, so a fresh buffer is zeroed or two images of one state would differ in what the allocator left there
            alloc = torch.zeros if self.controls else torch.empty
            out = alloc(self.state_bytes, dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous() or out.numel() != self.state_bytes:
            raise ValueError(f"out must be a contiguous uint8 tensor of {self.state_bytes} bytes on {self.device}")
        _lib.check(self._L.pcgrl_smb_state_export(self._handle(), out.data_ptr(), self._stream()), "pcgrl_smb_state_export")
        return out

    def get_rng_state(self):
        """uint64-as-int64 [N, 10]: both numpy-compatible PCG64 streams of every env (the layout of include/pcgrl_amd.h)."""
        out = torch.empty((self.num_envs, 10), dtype=torch.int64, device=self.device)
        _lib.check(self._L.pcgrl_smb_state_get_rng(self._handle(), out.data_ptr(), self._stream()), "pcgrl_smb_state_get_rng")
        return out

    def set_rng_state(self, rng, mask=None):
        r = self._dev(rng, torch.int64, (self.num_envs, 10))
        m = self._dev(mask, torch.uint8, (self.num_envs,))
        _lib.check(self._L.pcgrl_smb_state_set_rng(self._handle(), self._ptr(m), r.data_ptr(), self._stream()),
                   "pcgrl_smb_state_set_rng")

    def set_state(self, grids, pos, counters, ep_return, mask=None):
        """The inverse of get_state()'s first fields for the envs of `mask`: grids uint8 [N][H][W], pos int32 [N][2] (clamped to
        the map), counters int32 [N][4] = iteration, changes, n_step, searches, ep_return float64 [N].  Statistics and last_loss
        are recomputed from the maps; under a solver budget that may leave envs busy (env_busy()).  The last finished episode
        and the RNG streams stay as they are."""
        N = self.num_envs
        g = self._dev(grids, torch.uint8, (N,) + self.map_shape)
        p = self._dev(pos, torch.int32, (N, 2))
        c = self._dev(counters, torch.int32, (N, 4))
        r = self._dev(ep_return, torch.float64, (N,))
        m = self._dev(mask, torch.uint8, (N,))
        with torch.cuda.device(self.device):
            _lib.check(self._L.pcgrl_smb_state_set(self._handle(), self._ptr(m), g.data_ptr(), self._ptr(p), self._ptr(c),
                                                   self._ptr(r), self._stream()), "pcgrl_smb_state_set")

    def state_dict(self):
        """Everything needed to continue bit-exactly later: `blob` is export_state()'s image; the portable fields (maps,
        positions, counters = iteration, changes, n_step, searches, running returns, RNG streams) ride along."""
        N, dev = self.num_envs, self.device
        grids = torch.empty((N,) + self.map_shape, dtype=torch.uint8, device=dev)
        pos = torch.empty((N, 2), dtype=torch.int32, device=dev)
        counters = torch.empty((N, 4), dtype=torch.int32, device=dev)
        ep_return = torch.empty(N, dtype=torch.float64, device=dev)
        _lib.check(self._L.pcgrl_smb_env_get_state(self._handle(), grids.data_ptr(), pos.data_ptr(), counters.data_ptr(), None,
                                                   None, ep_return.data_ptr(), None, self._stream()), "pcgrl_smb_env_get_state")
        return {"grids": grids, "pos": pos, "counters": counters, "ep_return": ep_return, "rng": self.get_rng_state(),
                "blob": self.export_state()}

    def load_state_dict(self, sd, mask=None, index=None):
        """With "blob": the image import -- env j of `mask` (all without one) continues as row index[j] (j without an index) of
        the exporter; an image of another config or batch size is refused (ValueError), and so is a busy row for an env without
        a solver budget (NotImplementedError); nothing is overwritten then.  Without "blob": set_state and set_rng_state."""
        if "blob" in sd:
            b = self._dev(sd["blob"], torch.uint8)
            if b.dim() != 1 or b.numel() != self.state_bytes:
                raise ValueError(f"state_dict from an env with another config or batch size: the image has {b.numel()} bytes, "
                                 f"this env's has {self.state_bytes}")
            m = self._dev(mask, torch.uint8, (self.num_envs,))
            i = self._dev(index, torch.int32, (self.num_envs,))
            with torch.cuda.device(self.device):
                _lib.check(self._L.pcgrl_smb_state_import(self._handle(), self._ptr(m), self._ptr(i), b.data_ptr(),
                                                          self._stream()), "pcgrl_smb_state_import")
            return
        if index is not None:
            raise ValueError("index needs the image (\"blob\"): the portable fields are taken row for row")
        self.set_state(sd["grids"], sd["pos"], sd["counters"], sd["ep_return"], mask=mask)
        self.set_rng_state(sd["rng"], mask=mask)

    def set_solver_budget(self, budget):
        _refuse("a solver budget", "the play-through of this class is not resumable: a step launch lasts as long as its longest "
                "search (smb_ready.SmbReadyVecEnv, cfg.task.solver_budget, has the resumable one)")

    def step_ready(self, *args, **kw):
        _refuse("step_ready", "the play-through of this class is not resumable: a step launch lasts as long as its longest "
                "search (smb_ready.SmbReadyVecEnv, cfg.task.solver_budget, has the resumable one)")

    def check_errors(self):
        """Raises if a launch since the last check saw an action outside the space, a tile id above 6 or an import index outside
        the batch.  Synchronises."""
        _lib.check(self._L.pcgrl_smb_env_poll_error(self._handle()), "pcgrl_smb_env_poll_error")

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.pcgrl_smb_env_destroy(self._h)
            self._h = None
            self._workspace = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _get(cfg, path, default=None):
    cur = cfg
    for part in path.split("."):
        if cur is None:
            return default
        cur = cur.get(part, None) if isinstance(cur, dict) else getattr(cur, part, None)
    return default if cur is None else cur


def make_smb_vec_env(cfg, num_envs, device="cuda:0", seeds=None, auto_reset=True, sub_batches=1, reward_dtype=torch.float32):
    """make_vec_env's branch for cfg.task.problem == "smb"; everything outside narrow / turtle stepping is refused by name.
    cfg.controls with cfg.evaluate gives a controllable env; without cfg.evaluate it is refused.
    A positive cfg.task.solver_budget gives smb_ready.SmbReadyVecEnv (asynchronous stepping), absent or 0 an SmbVecEnv."""
    rep = _get(cfg, "representation")
    if rep == "wide":
        _refuse("the wide representation", "the reference's wide fails on a non-square map (wide_rep.py:42, IndexError)")
    controls = _get(cfg, "controls") or _get(cfg, "task.controls")
    if controls and not _get(cfg, "evaluate", False):
        # rl/envs.py:70-76: without cfg.evaluate the reference's make_env puts a target sampler on top of the ControlWrapper
        if _get(cfg, "task.alp_gmm", False):
            _refuse("controls with task.alp_gmm", "the ALP-GMM target sampler is outside the accelerated path: set cfg.evaluate "
                    "and queue targets, or use set_target_resampling")
        _refuse("controls without cfg.evaluate", "the reference's make_env then wraps UniformNoiseyTargets, which cannot be "
                "constructed at its commit (its __init__ reads self.num_params): set cfg.evaluate = True for the plain "
                "ControlWrapper -- targets through queue_targets -- and call set_target_resampling(True, seed) for that "
                "wrapper's effect")
    if _get(cfg, "static_prob") is not None or _get(cfg, "n_static_walls") is not None or _get(cfg, "static_tile_wrapper", False):
        _refuse("static tiles", "the static-tile wrapper is only on the 2-D engine")
    if _get(cfg, "act_window") is not None:
        _refuse("act_window", "action patches are only on the 2-D engine")
    if _get(cfg, "multiagent.n_agents", 0):
        _refuse("multiagent.n_agents", "multi-agent turtle stepping is only built for binary and zelda")
    if _get(cfg, "show_agents", False):
        _refuse("show_agents", "it needs the multi-agent wrapper")
    if (_get(cfg, "obs_format", "onehot") or "onehot") != "onehot":
        _refuse('obs_format="codes"', "the tile-code observation is only on the engine's problems")
    if int(sub_batches) > 1:
        _refuse("sub_batches > 1", "an env is one wave already, and the solver budget of smb_ready has nothing to overlap with")
    if _get(cfg, "n_aux_tiles", 0):
        _refuse("n_aux_tiles", "auxiliary tiles are outside the accelerated path")
    budget = _get(cfg, "task.solver_budget", 0)
    if isinstance(budget, bool) or int(budget) != budget or int(budget) < 0:
        raise ValueError(f"task.solver_budget must be a non-negative number of search iterations, got {budget!r}")
    kw = dict(device=device, obs_window=_get(cfg, "task.obs_window"), weights=_get(cfg, "task.weights"),
              max_board_scans=_get(cfg, "max_board_scans", 3), change_percentage=_get(cfg, "change_percentage"), seeds=seeds,
              auto_reset=auto_reset, solver_power=_get(cfg, "task.solver_power", 10000), reward_dtype=reward_dtype)
    if controls:  # (ControlWrapper(ctrl_metrics=cfg.controls) alone, cfg.evaluate: rewards in float64, as make_vec_env)
        kw.update(controls=list(controls), reward_dtype=torch.float64)
    if int(budget) > 0:
        from .smb_ready import SmbReadyVecEnv
        return SmbReadyVecEnv(rep, tuple(_get(cfg, "task.map_shape")), num_envs, solver_budget=int(budget), **kw)
    return SmbVecEnv(rep, tuple(_get(cfg, "task.map_shape")), num_envs, **kw)


class SmbGymEnv:
    """One Mario env with the reference's gym call shape on top of an SmbVecEnv of size 1: reset() -> (obs, {}), step(a) ->
    (obs float32 [oh][ow][8], reward, done, truncated, info).  info holds the nine statistics only on a step that changed the
    map (pcgrl_env.py:314-332), and always iterations, changes, max_iterations, max_changes.  With cfg.controls the observation
    is float32 [oh][ow][2K + 8], the 2K control values broadcast over planes in front (control_wrappers.py:189-214), and
    set_trgs(trgs) queues targets for the next reset."""

    metadata = {"render.modes": []}

    def __init__(self, cfg=None, vec=None, device="cuda:0", seed=None):
        from .envs import Box, Discrete
        self._vec = vec if vec is not None else make_smb_vec_env(cfg, 1, device=device, auto_reset=False,
                                                                 seeds=None if seed is None else [seed],
                                                                 reward_dtype=torch.float64)
        assert self._vec.num_envs == 1 and not self._vec.auto_reset
        v = self._vec
        self.ctrl_metrics = list(getattr(v, "controls", None) or [])
        shape = tuple(v.obs_shape[:-1]) + (v.obs_shape[-1] + 2 * len(self.ctrl_metrics),)
        self.observation_space = Box(low=0, high=1, shape=shape, dtype=np.float32)
        self.action_space = Discrete(v.num_actions)
        self.static_trgs = dict(v.spec.static_trgs)
        self.metric_trgs = self.static_trgs
        self.cond_bounds = dict(v.spec.cond_bounds)
        self._trg_queue = None
        self.metric_weights = dict(v.weights)
        self.metrics = {k: None for k in self.static_trgs}
        self._rep_stats = None
        self._changes = 0
        self.render_mode = None

    @property
    def unwrapped(self):
        return self

    def seed(self, seed=None):
        if seed is not None:
            self._vec.seed([int(seed)])
        return [seed]

    def _stats_dict(self, row):
        return {k: int(x) for k, x in zip(self._vec.stat_keys, row.tolist())}

    def set_trgs(self, trgs):
        """ControlWrapper.set_trgs: queued, applied at the next reset (a second call replaces the first)"""
        self._vec.queue_targets(dict(trgs))
        self._trg_queue = dict(trgs)

    def _obs_of(self, obs):
        o = obs[0].float().cpu().numpy()
        if not self.ctrl_metrics:
            return o
        c = self._vec.ctrl_obs[0].cpu().numpy()
        return np.concatenate((np.broadcast_to(c, o.shape[:-1] + c.shape), o), axis=-1)

    def reset(self, *, seed=None, options=None):
        if seed is not None:
            self.seed(seed)
        obs, _ = self._vec.reset()
        if self._trg_queue is not None:
            self.metric_trgs.update(self._trg_queue)
            self._trg_queue = None
        self._rep_stats = self._stats_dict(self._vec.get_state().stats[0].cpu())
        self.metrics = self._rep_stats
        self._changes = 0
        return self._obs_of(obs), {}

    def step(self, action):
        a = int(action)
        if not 0 <= a < self.action_space.n:
            raise IndexError(f"action {a} outside Discrete({self.action_space.n})")
        obs, rew, done, _, info = self._vec.step(torch.tensor([a], dtype=torch.int32, device=self._vec.device))
        self._rep_stats = self._stats_dict(info["stats"][0].cpu())
        self.metrics = self._rep_stats
        st = self._vec.get_state()
        changes = int(st.changes[0])
        out = dict(self._rep_stats) if changes != self._changes else {}
        self._changes = changes
        out.update(iterations=int(st.iteration[0]), changes=changes, max_iterations=int(self._vec.max_iterations),
                   max_changes=self._vec.max_changes)
        d = bool(done[0].item())
        return self._obs_of(obs), float(rew[0].item()), d, d, out

    def get_map(self):
        return self._vec.get_state().grids[0].cpu().numpy()

    @property
    def measures(self):
        """The behaviour characteristics of the current map under get_bc's names (evo/evolve.py:606-635) as Python floats, and
        "tile_fractions", get_counts' list (evolve.py:449-464): the dict PcgrlGymEnv.measures returns."""
        m = self._vec.measures()
        out = {k: float(v[0].item()) for k, v in m.bc.items()}
        out["tile_fractions"] = [float(x) for x in m.tile_fractions[0].cpu().tolist()]
        return out

    def close(self):
        self._vec.close()
