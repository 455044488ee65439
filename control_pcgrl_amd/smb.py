"""Super Mario Bros levels on the device: the nine statistics of SMBCtrlProblem.get_stats, the loss ControlWrapper.get_loss
derives from them and the A* play-through behind the play statistics, for a batch of maps in one launch
(include/pcgrl_amd_smb.h, csrc/smb/pcgrl_smb.h).

This module evaluates maps; smb_env.py steps SMB environments (SmbVecEnv) with the same kernels.  Neither is part of the 2-D
engine, so PROBLEMS / problem_spec / build_config do not know "smb".  file:line references are relative to the reference's control_pcgrl/ directory.
"""
import ctypes as C

import torch

from . import _lib
from .measures import MeasuresMixin
from .problems import ProblemSpec, target_interval

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
    spec = smb_spec(map_shape)
    weights = dict(spec.default_weights) if weights is None else dict(weights)
    unknown = set(weights) - set(spec.stat_keys)
    if unknown:
        raise ValueError(f"unknown smb statistics in weights: {sorted(unknown)}")
    cfg = _lib.PcgrlSmbConfig()
    cfg.h, cfg.w = int(map_shape[0]), int(map_shape[1])
    cfg.solver_power = int(solver_power)
    for i, k in enumerate(spec.stat_keys):
        lo, hi = target_interval(spec.static_trgs[k])
        cfg.has_trg[i] = 1
        cfg.weight[i] = float(weights.get(k, 0.0))
        cfg.trg_lo[i], cfg.trg_hi[i] = lo, hi
    return cfg


class SmbMeasures(MeasuresMixin):
    """Level measures and pairwise Hamming diversity of Mario maps on the device (include/pcgrl_amd_smb_measures.h, DESIGN.md
    section 24): what SmbEvaluator and SmbVecEnv share.  The result namespaces are field for field those of
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


class SmbEvaluator(SmbMeasures):
    """Evaluates batches of Mario maps on one device.  Owns the search workspace (a torch tensor of
    max_levels * (12 * (4 * solver_power + 1)) bytes, rounded up to 16 per level); batches above max_levels run as
    successive launches on the current stream.  There is no CPU fallback."""

    def __init__(self, map_shape=(16, 116), device="cuda:0", solver_power=10000, weights=None, max_levels=4096):
        self._L = _lib.lib()
        map_shape = tuple(int(s) for s in map_shape)
        if len(map_shape) != 2:
            raise ValueError(f"smb maps are 2-D, got shape {map_shape}")
        if int(max_levels) < 1:
            raise ValueError("max_levels must be at least 1")
        self.map_shape = map_shape
        self.spec = smb_spec(map_shape)
        self.solver_power = int(solver_power)
        self.max_levels = int(max_levels)
        self._cfg = smb_config(map_shape, solver_power, weights)
        nbytes = self._L.pcgrl_smb_workspace_bytes(self.max_levels, map_shape[0], map_shape[1], self.solver_power)
        if nbytes < 0:
            raise NotImplementedError(
                f"smb: map_shape {map_shape} / solver_power {solver_power} outside {MIN_H}..{MAX_H} x 1..{MAX_W} and "
                f"1..{MAX_SOLVER_POWER}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("SmbEvaluator needs a cuda device: there is no CPU fallback")
        self._workspace = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)
        self._workspace_bytes = nbytes
        self._error = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def evaluate(self, grids, cap=512, jump_cap=64, playthrough=True):
        """grids: uint8 [n][H][W] (a device tensor, or anything torch.as_tensor takes).  Returns device tensors:
        stats int32 [n][9] (spec.stat_keys order), loss float64 [n], won bool [n], play int32 [n][6] (won, x, y, airTime,
        iterations of pass 1, of pass 2), and with playthrough: moves int8 [n][cap], length int32 [n], jump_locs
        int16 [n][jump_cap][2]."""
        if self._workspace is None:
            raise RuntimeError("SmbEvaluator is closed")
        g = torch.as_tensor(grids, device=self.device)
        if g.dtype != torch.uint8:
            g = g.to(torch.uint8)
        if g.dim() == 2:
            g = g.unsqueeze(0)
        if g.dim() != 3 or tuple(g.shape[1:]) != self.map_shape:
            raise ValueError(f"grids must have shape [n]{list(self.map_shape)}, got {list(g.shape)}")
        g = g.contiguous()
        n = g.shape[0]
        if n < 1:
            raise ValueError("no levels to evaluate")
        cap, jump_cap = int(cap), int(jump_cap)
        if playthrough and (cap < 1 or jump_cap < 1):
            raise ValueError("cap and jump_cap must be at least 1")
        dev = self.device
        out = {"stats": torch.empty((n, 9), dtype=torch.int32, device=dev),
               "loss": torch.empty(n, dtype=torch.float64, device=dev),
               "play": torch.empty((n, 6), dtype=torch.int32, device=dev)}
        if playthrough:
            out["moves"] = torch.empty((n, cap), dtype=torch.int8, device=dev)
            out["length"] = torch.empty(n, dtype=torch.int32, device=dev)
            out["jump_locs"] = torch.empty((n, jump_cap, 2), dtype=torch.int16, device=dev)
        err = torch.empty(n, dtype=torch.int32, device=dev)

        def ptr(name, lo):
            return out[name][lo:].data_ptr() if name in out else None

        with torch.cuda.device(dev):
            stream = self._stream()
            for lo in range(0, n, self.max_levels):
                m = min(self.max_levels, n - lo)
                _lib.check(self._L.pcgrl_smb_evaluate(
                    C.byref(self._cfg), m, g[lo:].data_ptr(), self._workspace.data_ptr(), self._workspace_bytes, cap, jump_cap,
                    ptr("stats", lo), ptr("loss", lo), ptr("moves", lo), ptr("length", lo), ptr("jump_locs", lo),
                    ptr("play", lo), err[lo:].data_ptr(), stream), "pcgrl_smb_evaluate")
        self._error |= err.max()
        out["won"] = out["play"][:, 0] != 0
        return out

    def measures(self, grids, entropy=True):
        """The behaviour characteristics of the maps that the reference computes from the integer map (evo/evolve.py:606-635
        get_bc -> :423-592), as VecPcgrlEnv.measures returns them with T = 7: counts int32 [n, 7], match int32 [n, 3]
        (horizontal, vertical, wrapped co-occurance matches), tile_fractions float64 [n, 7] and bc, a dict under get_bc's names
        -> float64 [n] (also .entropy, .emptiness).  All but entropy equal the reference bit for bit; entropy does on the host
        whose numpy built the table.  grids: uint8 [n][H][W] at any alignment, n >= 0; ids are masked to 3 bits and set no
        error.  One launch on the current stream, no host sync."""
        g = self._grids_arg(grids)
        return self._measures(None, g.shape[0], g, entropy)

    def diversity(self, grids, group=None, pairwise=False):
        """Pairwise Hamming distances (cells whose tiles differ) among the maps in consecutive groups of `group` maps (None: one
        group of all), as VecPcgrlEnv.diversity returns them: hamming_sum int64 [G], nearest / nearest_idx int32 [n] (the lowest
        index on ties), div_score (rl/evaluate_ctrl.py:42-48) and diversity_bonus (evo/evolve.py:1236-1244) float64 [G],
        pairwise int32 [G, K, K] or None.  Three launches on the current stream, no host sync."""
        g = self._grids_arg(grids)
        return self._diversity(None, g.shape[0], g, group, pairwise)

    def check_errors(self):
        """Raises if a launch since the last check read a tile id above 6 (it was taken as empty).  Synchronises."""
        bits = int(self._error.item())
        self._error.zero_()
        if bits & 1:
            raise ValueError("smb: a tile id above 6 was seen on the device (read as empty)")

    def close(self):
        self._workspace = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
