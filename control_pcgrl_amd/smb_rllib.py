"""Super Mario Bros behind ray.rllib's `VectorEnv` call shape: `SmbVectorEnv`, what rllib_env.PcgrlVectorEnv is for the
engine's problems -- one SmbVecEnv for a worker's whole batch, one step launch per `vector_step`, the arrays of a call in a
pinned host block of their own that nothing writes again.

    register_env("pcgrl", lambda c: make_vector_env(c, c["num_envs_per_worker"]))   # every problem, smb included

The observation is large (stock 32 x 232 window: 59 392 bytes per env as uint8, 356 352 as the float32 of RLlib's Box with two
controls), so the float32 form is not converted from the uint8 one: the step runs with no observation output, and a kernel of
its own (include/pcgrl_amd_smb_vector.h) writes the final float32 image -- control planes in front -- once, straight into the
block the caller receives (`direct_host_outputs`) or into the one device block the call's single copy moves.

    obs_dtype=np.float32   Box [oh, ow, 2K + 8] (default; forced with controls)
    obs_dtype=np.uint8     the step / reset kernels' own bytes, [oh, ow, 8] (no controls): a quarter of the traffic, the
                           form for large batches

Rewards are handed out from the float64 output in both forms.  Episode ends follow RLlib's contract as PcgrlVectorEnv does:
`vector_step` returns the true last observation of a finished episode, and all envs that finished in one step are reset by one
masked launch on the first `reset_at`.  A `VectorEnv` step is synchronous, so a solver budget is refused.  Sub-batches
(make_vec_env's `sub_batches`, refused for smb there) have no argument here at all: passing one is a TypeError.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from . import rllib_env
from .envs import Box, Discrete
from .rllib_env import _Base, _VectorAdapter, _hip_runtime
from .smb_env import SmbVecEnv, _get
from .vec_env import make_vec_env

N_STATS = 9


def block_layout(num_envs, obs_bytes):
    """The packed block of one call: [obs | reward64 | stats | done], every section on 16 bytes.  obs_bytes: one env's
    observation as handed out.  Returns the sections' offsets and the block's size."""
    def up(x):
        return (x + 15) & ~15

    N = int(num_envs)
    o_rew = up(N * int(obs_bytes))
    o_stats = o_rew + up(N * 8)
    o_done = o_stats + up(N * N_STATS * 4)
    return SimpleNamespace(obs=0, rew=o_rew, stats=o_stats, done=o_done, total=o_done + up(N))


def _refuse(what, why):
    raise NotImplementedError(f"SmbVectorEnv: {what} is refused: {why}")


def _refuse_budget(budget):
    _refuse(f"a solver budget (task.solver_budget / SmbReadyVecEnv.solver_budget = {budget})", "a VectorEnv step is "
            "synchronous -- it returns every env's result -- and under a budget an env may answer \"busy\", its committed state "
            "not being the state of the step in flight: leave the budget out or set_solver_budget(0) first "
            "(SmbReadyVecEnv.step_ready has the asynchronous form)")


class SmbVectorEnv(_VectorAdapter, _Base):
    DIRECT_MAX_BYTES = rllib_env.PcgrlVectorEnv.DIRECT_MAX_BYTES  # the kernels write into host memory themselves up to here

    def __init__(self, cfg=None, num_envs=1, device="cuda:0", seeds=None, vec: SmbVecEnv = None, obs_dtype=np.float32,
                 direct_host_outputs=None):
        if vec is None:
            if _get(cfg, "task.problem") != "smb":
                raise ValueError(f"SmbVectorEnv serves task.problem == 'smb', got {_get(cfg, 'task.problem')!r}: "
                                 "PcgrlVectorEnv has the engine's problems (make_vector_env picks the class)")
            budget = _get(cfg, "task.solver_budget", 0)
            try:  # (a numpy number or a numeric string too; what is no number at all is make_vec_env's to name)
                positive = not isinstance(budget, bool) and float(budget) > 0
            except (TypeError, ValueError):
                positive = False
            if positive:
                _refuse_budget(budget)
            vec = make_vec_env(cfg, num_envs, device=device, seeds=seeds, auto_reset=False)  # (refuses what smb cannot do)
            if int(getattr(vec, "solver_budget", 0) or 0) > 0:  # (however the cfg spelt it: never an env that can answer "busy")
                budget = vec.solver_budget
                vec.close()
                _refuse_budget(budget)
        elif int(getattr(vec, "solver_budget", 0) or 0) > 0:
            _refuse_budget(vec.solver_budget)
        if vec.auto_reset:
            _refuse("a vec built with auto_reset=True", "the adapter drives resets itself (RLlib calls reset_at) and returns "
                    "the true last observation of a finished episode: build the SmbVecEnv with auto_reset=False")
        self.vec = v = vec
        self.num_envs = N = v.num_envs
        self.n_ctrl_planes = 2 * len(v.controls)
        self.obs_dtype = np.dtype(obs_dtype if not self.n_ctrl_planes else np.float32)  # (control planes are fractions)
        if self.obs_dtype not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise ValueError("obs_dtype must be float32 (the reference's declared Box dtype) or uint8 (the step kernel's bytes)")
        self._f32 = self.obs_dtype == np.dtype(np.float32)
        shape = tuple(v.obs_window) + (self.n_ctrl_planes + v.obs_shape[-1],)
        if self.n_ctrl_planes:  # (declared [0, 1] by the reference too although target / range can leave the interval)
            self.observation_space = Box(low=np.zeros(shape, np.float32), high=np.ones(shape, np.float32), dtype=np.float32)
        else:
            self.observation_space = Box(low=0, high=1, shape=shape, dtype=np.float32)
        self.action_space = Discrete(v.num_actions)
        if _Base is not object:  # pragma: no cover
            super().__init__(self.observation_space, self.action_space, N)
        self._out_shape = (N,) + shape
        self._lay = lay = block_layout(N, int(np.prod(shape)) * self.obs_dtype.itemsize)
        self._total = lay.total
        if direct_host_outputs is None:
            direct_host_outputs = lay.total <= self.DIRECT_MAX_BYTES
        self._direct = bool(direct_host_outputs)
        self._hip = _hip_runtime()
        self._act = torch.zeros(N, dtype=torch.int32).pin_memory()
        self._act_np = self._act.numpy()
        if self._direct:  # the kernels read the actions from, and write every output into, pinned host memory themselves
            self._dev, self._act_dev = None, self._act
        else:
            self._dev = torch.zeros(lay.total, dtype=torch.uint8, device=v.device)
            self._act_dev = torch.zeros(N, dtype=torch.int32, device=v.device)
        self._adapter_state()

    # -- helpers -----------------------------------------------------------------------------------
    def _views(self, lease):
        """numpy views of a call's block (they keep the lease, and so the block, alive)"""
        h, lay, N = np.asarray(lease), self._lay, self.num_envs
        nb = int(np.prod(self._out_shape)) * self.obs_dtype.itemsize
        return dict(obs=h[:nb].view(self.obs_dtype).reshape(self._out_shape), rew=h[lay.rew:lay.rew + N * 8].view(np.float64),
                    stats=h[lay.stats:lay.stats + N * N_STATS * 4].view(np.int32).reshape(N, N_STATS),
                    done=h[lay.done:lay.done + N].view(np.bool_))

    def _out_ptrs(self, lease):
        b, lay = (lease.ptr if self._direct else self._dev.data_ptr()), self._lay
        return b, b + lay.rew, b + lay.stats, b + lay.done

    def _finish(self, lease, stream):
        """the call's one device -> host copy (unless the kernels wrote into the block themselves), and the wait"""
        if not self._direct:
            rc = self._hip.pcgrl_copy_to_host(lease.ptr, self._dev.data_ptr(), self._total, stream)
            if rc:
                _lib.check(rc, "pcgrl_copy_to_host")
        rc = self._hip.pcgrl_stream_synchronize(stream)
        if rc:
            _lib.check(rc, "pcgrl_stream_synchronize")

    def _masked_reset(self, mask):
        """one launch for every env in `mask`; the observations go to a block of their own and, for the masked envs only,
        the statistics into the current ones"""
        v = self.vec
        m = torch.as_tensor(mask.astype(np.uint8), device=v.device)
        s = v._stream()
        lease = self._lease()
        obs_p, _, stats_p, _ = self._out_ptrs(lease)
        _lib.check(v.reset_masked(m.data_ptr(), s, obs_ptr=None if self._f32 else obs_p), "pcgrl_smb_env_reset")
        if self._f32:
            _lib.check(v.observe_f32_into(obs_p, s), "pcgrl_smb_env_observe_f32")
        _lib.check(v.stats_into(stats_p, s), "pcgrl_smb_env_get_state")
        self._finish(lease, s)
        self._took_reset(mask, self._views(lease))

    def vector_step(self, actions):
        v = self.vec
        a = np.asarray(actions, dtype=np.int64).reshape(self.num_envs)
        if a.min() < 0 or a.max() >= v.num_actions:
            raise IndexError("action outside the action space")  # the reference raises IndexError from numpy indexing
        self._act_np[...] = a
        s = v._stream()
        if not self._direct:
            self._act_dev.copy_(self._act, non_blocking=True)
        lease = self._lease()
        obs_p, rew_p, stats_p, done_p = self._out_ptrs(lease)
        rc = v.step_into(self._act_dev.data_ptr(), None if self._f32 else obs_p, None, rew_p, done_p, stats_p, s)
        if rc:
            _lib.check(rc, "pcgrl_smb_env_step")
        if self._f32:  # the final image, once: the step wrote no observation
            rc = v.observe_f32_into(obs_p, s)
            if rc:
                _lib.check(rc, "pcgrl_smb_env_observe_f32")
        self._finish(lease, s)
        return self._took_step(self._views(lease))


def make_vector_env(cfg, num_envs, **kw):
    """The VectorEnv adapter of cfg's problem: SmbVectorEnv for task.problem == "smb", PcgrlVectorEnv otherwise."""
    if _get(cfg, "task.problem") == "smb":
        return SmbVectorEnv(cfg, num_envs, **kw)
    return rllib_env.PcgrlVectorEnv(cfg, num_envs, **kw)
