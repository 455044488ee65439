"""Asynchronous stepping of Super Mario Bros environments: SmbVecEnv under a solver budget (include/pcgrl_amd_smb_ready.h,
csrc/smb/pcgrl_smb_ready.h).

SmbVecEnv.step lasts as long as the longest A* play-through of its launch.  Here a launch gives every env at most `solver_budget`
search iterations; a search that does not finish is parked on the device and continues in the next launch, and info["status"]
tells per env what happened: STATUS_EMITTED -- the env completed a step in this launch and its reward / done / stats rows are
valid -- and STATUS_BUSY -- the env is busy after this launch and ignores the next launch's action.  Per-env trajectories are
exactly SmbVecEnv's, only later.  tests/smb_ready_rules.py has the launch rules in plain Python.
"""
import ctypes as C

import torch

from . import _lib
from .smb_env import SmbVecEnv

STATUS_EMITTED, STATUS_BUSY = 1, 2  # PCGRL_ENV_EMITTED, PCGRL_ENV_BUSY of include/pcgrl_amd.h


class SmbReadyVecEnv(SmbVecEnv):
    """SmbVecEnv with a resumable play-through.  step_ready(actions) -> step()'s tuple with info["status"] uint8 [N]; env i takes
    actions[i] iff it was not busy after the previous launch (after a reset: env_busy()), and every emitted transition belongs to
    the last action the env took.  The observation rows are written for every env in every launch: a busy env's row is the
    observation of the step in flight.  reset() runs the new levels' searches under the budget too and may leave envs busy;
    get_state() returns the committed state -- for an env with a step in flight, the state before that step.  With controls
    the queued or resampled targets are committed by the launch that draws or injects the new level; an env's ctrl_obs row shows
    the new level's statistic once its search is over (until then the old level's)."""

    def __init__(self, representation, map_shape=(16, 116), num_envs=1, solver_budget=256, **kw):
        budget = int(solver_budget)
        if budget < 1:
            raise ValueError(f"solver_budget must be a positive number of search iterations per launch, got {solver_budget!r}")
        super().__init__(representation, map_shape, num_envs, **kw)
        self._status = torch.empty(self.num_envs, dtype=torch.uint8, device=self.device)
        self._busy = torch.empty(self.num_envs, dtype=torch.uint8, device=self.device)
        self._step_out = (self._obs, self._reward, self._done, self._done,
                          dict(self._step_out[4], stats=self._stats, status=self._status))
        self.park_bytes = int(self._L.pcgrl_smb_ready_park_bytes(C.byref(self.cfg)))
        self.set_solver_budget(budget)

    @property
    def solver_budget(self):
        return int(self._L.pcgrl_smb_ready_get_budget(self._handle()))

    def set_solver_budget(self, budget):
        """Search iterations per env and launch from the next launch on; parked searches continue under the new budget.  0 goes
        back to synchronous stepping (step()), which is refused while an env is busy."""
        with torch.cuda.device(self.device):
            _lib.check(self._L.pcgrl_smb_ready_set_budget(self._handle(), int(budget)), "pcgrl_smb_ready_set_budget")

    def step(self, actions):
        if self.solver_budget > 0:
            raise RuntimeError("SmbReadyVecEnv.step: a solver budget is set and step() cannot say which envs are busy: use "
                               "step_ready(), or set_solver_budget(0) once no env is busy")
        return super().step(actions)

    def rollout(self, *args, **kw):
        if self.solver_budget > 0:
            raise NotImplementedError("SmbReadyVecEnv.rollout: a solver budget is set and a rollout cannot say which envs are "
                                      "busy: K steps in one launch run every search to its end.  Use step_ready(), or "
                                      "set_solver_budget(0) once no env is busy")
        return super().rollout(*args, **kw)

    def step_ready(self, actions):
        if actions.numel() != self.num_envs:
            raise ValueError(f"actions must be [{self.num_envs}], got {tuple(actions.shape)}")
        if actions.dtype != torch.int32 or not actions.is_contiguous() or actions.device != self.device:
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        rc = self._L.pcgrl_smb_ready_step(self._handle(), actions.data_ptr(), 1 if self.auto_reset else 0, self._obs.data_ptr(),
                                          self._r32, self._r64, self._done.data_ptr(), self._stats.data_ptr(),
                                          self._status.data_ptr(), self._stream())
        if rc:
            _lib.check(rc, "pcgrl_smb_ready_step")
        return self._step_out

    def env_busy(self):
        """uint8 [N]: 1 = the env is busy now -- what the last launch's STATUS_BUSY said, or what a reset left behind."""
        _lib.check(self._L.pcgrl_smb_ready_busy(self._handle(), self._busy.data_ptr(), self._stream()), "pcgrl_smb_ready_busy")
        return self._busy
