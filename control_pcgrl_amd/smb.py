"""Super Mario Bros levels on the device: the nine statistics of SMBCtrlProblem.get_stats, the loss ControlWrapper.get_loss
derives from them and the A* play-through behind the play statistics, for a batch of maps in one launch
(include/pcgrl_amd_smb.h, csrc/smb/pcgrl_smb.h).

This module evaluates maps; smb_env.py steps SMB environments (SmbVecEnv) with the same kernels.  Neither is part of the 2-D
engine, so PROBLEMS / problem_spec / build_config do not know "smb".  file:line references are relative to the reference's control_pcgrl/ directory.
"""
import torch

from . import _lib
from .evaluator import LevelEvaluator
from .measures import MeasuresMixin
from .problems import ProblemSpec, fill_targets

SMB_TILES = ["empty", "solid", "enemy", "brick", "question", "coin", "tube"]  # envs/probs/smb/smb_prob.py:12
SMB_STAT_KEYS = ["dist-floor", "disjoint-tubes", "enemies", "empty", "noise", "jumps", "jumps-dist", "dist-win", "sol-length"]
SMB_MOVES = ((0, 0), (1, 0), (0, -1), (1, -1))  # smb/engine.py:3, (dx, dy)
MIN_H, MAX_H, MAX_W, MAX_SOLVER_POWER = 4, 16, 128, 16000


def smb_spec(map_shape=(16, 116)) -> ProblemSpec:
    """smb_prob.py:16-26 sets _width = 116, _height = 16 BEFORE smb_ctrl_prob.py:8-36 derive the targets and bounds, so those
    are frozen at the stock size whatever the map (adjust_param moves _width / _height to the map's afterwards)."""
    fw, fh = 116, 16
    n = fw * fh
    max_sol = float(fw * 3)
    return ProblemSpec(
        "smb", list(SMB_TILES), list(SMB_STAT_KEYS),
        {"dist-floor": 0, "disjoint-tubes": 0, "enemies": (10, 30), "empty": (900, n), "noise": 0, "jumps": (20, n),
         "jumps-dist": 0, "dist-win": 0, "sol-length": max_sol},
        {"dist-floor": (0, n), "disjoint-tubes": (0, n), "enemies": (0, n), "empty": (0, fw), "noise": (0, n), "jumps": (0, fw),
         "jumps-dist": (0, n), "dist-win": (0, fw), "sol-length": (0, max_sol)},
        {"dist-floor": 2, "disjoint-tubes": 1, "enemies": 1, "empty": 1, "noise": 4, "jumps": 2, "jumps-dist": 2, "dist-win": 5,
         "sol-length": 1},  # configs/config.py:115-139 SMBConfig
        {"dist-floor": 2, "disjoint-tubes": 1, "enemies": 1, "empty": 1, "noise": 4, "jumps": 2, "jumps-dist": 2, "dist-win": 5,
         "sol-length": 1},  # smb_prob.py:28-38
    )


def smb_config(map_shape=(16, 116), solver_power=10000, weights=None) -> "_lib.PcgrlSmbConfig":
    """The C config of include/pcgrl_amd_smb.h: the frozen targets as zero-loss intervals, and the weights."""
    cfg = _lib.PcgrlSmbConfig()
    cfg.h, cfg.w = int(map_shape[0]), int(map_shape[1])
    cfg.solver_power = int(solver_power)
    return fill_targets(cfg, smb_spec(map_shape), weights, "smb statistics")


class SmbMeasures(MeasuresMixin):
    """Level measures and pairwise Hamming diversity of Mario maps on the device (include/pcgrl_amd_smb_measures.h, DESIGN.md
    section 24) for SmbVecEnv (SmbEvaluator reaches the caller-map entry points through LevelEvaluator).  The result namespaces are field for field those of
    VecPcgrlEnv.measures / .diversity, with T = 7.  A user class has map_shape, device, _L and _stream(); `h` is an env handle
    whose committed maps are read, or None with caller maps."""

    def _meas_dims(self):
        return self.map_shape[0] * self.map_shape[1], len(SMB_TILES)

    def _grids_arg(self, grids):
        g = torch.as_tensor(grids, device=self.device)
        if g.dtype != torch.uint8:
            g = g.to(torch.uint8)
        if g.dim() == 2:
            g = g.unsqueeze(0)
        if g.dim() != 3 or tuple(g.shape[1:]) != tuple(self.map_shape):
            raise ValueError(f"grids must have shape [n]{list(self.map_shape)}, got {list(g.shape)}")
        return g.contiguous()

    def _measures(self, h, n, grids, entropy):
        if h is not None:
            return self._measures_result(self._L.pcgrl_smb_env_measures, (h,), n, entropy)
        return self._measures_result(self._L.pcgrl_smb_measures_for_grids, (*self.map_shape, n, grids.data_ptr()), n, entropy)

    def _diversity(self, h, n, grids, group, pairwise):
        fn, head = self._L.pcgrl_smb_env_diversity, (h,)
        if h is None:
            fn, head = self._L.pcgrl_smb_diversity_for_grids, (*self.map_shape, n, grids.data_ptr())
        return self._diversity_result(fn, head, n, group, pairwise,
                                      self._L.pcgrl_smb_diversity_scratch_bytes(*self.map_shape, n))


class SmbEvaluator(LevelEvaluator):
    """Evaluates batches of Mario maps on one device.  Owns the search workspace (a torch tensor of
    max_levels * (12 * (4 * solver_power + 1)) bytes, rounded up to 16 per level); batches above max_levels run as
    successive launches on the current stream.  There is no CPU fallback.  measures() and diversity() are the base's with
    T = 7 (include/pcgrl_amd_smb_measures.h, DESIGN.md section 24: the entry points SmbMeasures gives SmbVecEnv)."""

    NAME, TILES, STAT_KEYS, TILE_READ_AS = "smb", SMB_TILES, SMB_STAT_KEYS, "empty"
    behaviour = None  # not built for smb: there is no table of names to place a level by

    def __init__(self, map_shape=(16, 116), device="cuda:0", solver_power=10000, weights=None, max_levels=4096):
        super().__init__(map_shape, max_levels)
        map_shape = self.map_shape
        self.spec = smb_spec(map_shape)
        self.solver_power = int(solver_power)
        self._cfg = smb_config(map_shape, solver_power, weights)
        nbytes = self._L.pcgrl_smb_workspace_bytes(self.max_levels, map_shape[0], map_shape[1], self.solver_power)
        if nbytes < 0:
            raise NotImplementedError(
                f"smb: map_shape {map_shape} / solver_power {solver_power} outside {MIN_H}..{MAX_H} x 1..{MAX_W} and "
                f"1..{MAX_SOLVER_POWER}")
        self._open(device)
        self._workspace = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)
        self._workspace_bytes = nbytes

    def evaluate(self, grids, cap=512, jump_cap=64, playthrough=True):
        """grids: uint8 [n][H][W] (a device tensor, or anything torch.as_tensor takes).  Returns device tensors:
        stats int32 [n][9] (spec.stat_keys order), loss float64 [n], won bool [n], play int32 [n][6] (won, x, y, airTime,
        iterations of pass 1, of pass 2), and with playthrough: moves int8 [n][cap], length int32 [n], jump_locs
        int16 [n][jump_cap][2]."""
        g = self._levels_arg(grids)
        n, dev = g.shape[0], self.device
        cap, jump_cap = int(cap), int(jump_cap)
        if playthrough and (cap < 1 or jump_cap < 1):
            raise ValueError("cap and jump_cap must be at least 1")
        out = {"stats": torch.empty((n, 9), dtype=torch.int32, device=dev),
               "loss": torch.empty(n, dtype=torch.float64, device=dev),
               "play": torch.empty((n, 6), dtype=torch.int32, device=dev)}
        if playthrough:
            out["moves"] = torch.empty((n, cap), dtype=torch.int8, device=dev)
            out["length"] = torch.empty(n, dtype=torch.int32, device=dev)
            out["jump_locs"] = torch.empty((n, jump_cap, 2), dtype=torch.int16, device=dev)
        self._launch(self._call("evaluate"), g, (self._workspace.data_ptr(), self._workspace_bytes, cap, jump_cap), out,
                     ("stats", "loss", "moves", "length", "jump_locs", "play"))
        out["won"] = out["play"][:, 0] != 0
        return out
