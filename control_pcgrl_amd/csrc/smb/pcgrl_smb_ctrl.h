// smb/pcgrl_smb_ctrl.h -- controllable generation for Super Mario Bros environments (include/pcgrl_amd_smb_ctrl.h): per-env
// targets in HBM, queued targets that take effect at the env's next reset, the control observation and device-side target
// resampling.  DESIGN.md section 22 has the rules; tests/smb_ctrl_rules.py is the same in plain Python.
//
//   record    SmbCtrlRec, one per env: the active zero-loss interval of all nine statistics, per control j the value the control
//             observation shows, the queued (lo, hi, observed) triple, the set of controls the queue names, and a flag word --
//             bit 0 = targets are queued, bits 1.. = the resets that resampled this env's targets so far (the draw counter).
//   config    SmbCtrlCfg, one per handle, in HBM too: the control list and ranges, and the resampling switch, seed and bounds,
//             which pcgrl_smb_ctrl_set_resampling writes in stream order (a captured launch sees the change).
//   kernels   every kernel family that computes a loss has a controllable instantiation (template <bool CTRL>).  It loads the
//             27 doubles of the record's active part and the flag word into LDS (SmbCtrlLds) next to the state record's load, so
//             the loads drain under the map load; the loss reads the LDS copy.
//   take      at a reset, before the new level's last_loss: lane j < n_ctrl takes control j's queued triple (if the queue names
//             it) or its resampled target, and writes it to LDS and to the record; lane 0 stores the flag word.  One commit per
//             reset; the LDS copy is what the rest of the launch reads, so a rollout never reads its own stores back.
//   loss      smb_target_loss of smb/pcgrl_smb.h, the one every loss goes through, against the LDS copy of the targets.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcgrl_smb.h"

namespace pcgrl {

struct alignas(16) SmbCtrlRec {
  double lo[SMB_STATS], hi[SMB_STATS];  // active, per statistic
  double obs[SMB_STATS];                // per control j: the target value the control observation shows
  double q[SMB_STATS][3];               // per control j: queued lo, hi, observed value
  int32_t flag;                         // bit 0: queued targets wait; bits 1..: the draw counter
  int32_t qmask;                        // bit j: the queue names control j
  int32_t pad[2];
};
static_assert(sizeof(SmbCtrlRec) == 448, "SmbCtrlRec layout");
constexpr int SMB_CTRL_ACTIVE = 3 * SMB_STATS;  // the doubles every kernel loads: lo, hi, obs

struct SmbCtrlCfg {
  int32_t n_ctrl, enable;  // enable: resample at every reset
  uint64_t seed;
  int32_t idx[SMB_STATS];  // control j is statistic idx[j]
  int32_t pad;
  double range[SMB_STATS], rs_lo[SMB_STATS], rs_hi[SMB_STATS];  // per control j
};

// what the env kernels see of a controllable handle (all null otherwise)
struct SmbCtrlArgs {
  const SmbCtrlCfg *cfg;
  SmbCtrlRec *rec;  // [n]
  float *obs;       // [n][2 * n_ctrl], or null
};

// the small kernels of include/pcgrl_amd_smb_ctrl.h
struct SmbCtrlQueueArgs {
  int32_t n, n_named;
  int32_t named[SMB_STATS];  // control indices j, in the caller's order
  SmbCtrlRec *rec;
  const uint8_t *mask;
  const double *lo, *hi, *obs;  // [n][n_named]
};
struct SmbCtrlGetArgs {
  int32_t n;
  const SmbCtrlRec *rec;
  double *active;   // [n][9][2]
  double *shown;    // [n][9]
  double *queued;   // [n][9][3]
  int32_t *flags;   // [n][2]: flag word, queue set
};
struct SmbCtrlObserveArgs {
  int32_t n;
  SmbCtrlArgs c;
  const int32_t *stats;  // the state records' statistics: [n] records of `stats_stride` bytes, the row at `stats_offset`
  int64_t stats_stride, stats_offset;
};
struct SmbCtrlResampleArgs {
  SmbCtrlCfg *cfg;
  int32_t enable, n_ctrl;
  uint64_t seed;
  double lo[SMB_STATS], hi[SMB_STATS];
};

hipError_t launch_smb_ctrl_queue(const SmbCtrlQueueArgs &a, hipStream_t s);
hipError_t launch_smb_ctrl_get(const SmbCtrlGetArgs &a, hipStream_t s);
hipError_t launch_smb_ctrl_observe(const SmbCtrlObserveArgs &a, hipStream_t s);
hipError_t launch_smb_ctrl_resample(const SmbCtrlResampleArgs &a, hipStream_t s);

#ifdef PCGRL_KERNEL_TU
}  // namespace pcgrl
#include "../pcgrl_kernels2d.h"  // trg_resampled
namespace pcgrl {

// the active part of an env's record in LDS; the empty form costs the plain kernels nothing
struct SmbCtrlLds {
  double v[SMB_CTRL_ACTIVE];  // lo[9], hi[9], obs[9]
  int32_t flag;
};
struct SmbCtrlNone {};
template <bool CTRL>
struct SmbCtrlLdsOf {
  using type = SmbCtrlNone;
};
template <>
struct SmbCtrlLdsOf<true> {
  using type = SmbCtrlLds;
};

// issued with the state record's load at the top of a kernel; visible after the kernel's next barrier
__device__ __forceinline__ void smb_ctrl_load(SmbCtrlLds &C, const SmbCtrlArgs &c, int env, int lane) {
  const SmbCtrlRec *R = c.rec + env;
  if (lane < SMB_CTRL_ACTIVE) C.v[lane] = ((const double *)R)[lane];
  if (lane == SMB_CTRL_ACTIVE) C.flag = R->flag;
}
__device__ __forceinline__ void smb_ctrl_load(SmbCtrlNone &, const SmbCtrlArgs &, int, int) {}

// A reset takes the queued or resampled targets (control_wrappers.py:174-178, :453-471) before the new level's loss.  Every
// lane calls it, after a barrier that follows smb_ctrl_load and every earlier read of C; it ends with a barrier.
__device__ inline void smb_ctrl_take(SmbCtrlLds &C, const SmbCtrlArgs &c, int env, int lane) {
  const SmbCtrlCfg &cc = *c.cfg;
  SmbCtrlRec *R = c.rec + env;
  const int32_t flag = C.flag;
  const bool resample = cc.enable != 0, pending = (flag & 1) != 0;
  if (resample || pending) {
    if (lane < cc.n_ctrl) {
      const int j = lane, k = cc.idx[j];
      bool take = false;
      double lo = 0.0, hi = 0.0, ob = 0.0;
      if (resample) {
        lo = hi = ob = trg_resampled(cc.seed, env, (uint32_t)flag >> 1, j, cc.rs_lo[j], cc.rs_hi[j]);
        take = true;
      } else if ((R->qmask >> j) & 1) {
        lo = R->q[j][0], hi = R->q[j][1], ob = R->q[j][2];
        take = true;
      }
      if (take) {
        C.v[k] = R->lo[k] = lo;
        C.v[SMB_STATS + k] = R->hi[k] = hi;
        C.v[2 * SMB_STATS + j] = R->obs[j] = ob;
      }
    }
    __syncthreads();  // (uniform: every lane holds the same flag and switch)
    if (lane == 0) C.flag = R->flag = resample ? (int32_t)((((uint32_t)flag >> 1) + 1u) << 1) : (flag & ~1);
  }
  __syncthreads();
}
__device__ __forceinline__ void smb_ctrl_take(SmbCtrlNone &, const SmbCtrlArgs &, int, int) {}

// ControlWrapper.get_loss with the env's own targets
__device__ __forceinline__ double smb_ctrl_loss(const SmbCtrlLds &C, const int32_t *has_trg, const double *weight,
                                                const int32_t *stats) {
  return smb_target_loss(has_trg, weight, C.v, C.v + SMB_STATS, stats);
}

// control_wrappers.py:189-214: (target / range, metric / range) per control, as float32; lanes j < n_ctrl write
__device__ __forceinline__ void smb_ctrl_write_obs(const SmbCtrlLds &C, const SmbCtrlArgs &c, int row, int lane,
                                                   const int32_t *stats) {
  if (!c.obs) return;
  const SmbCtrlCfg &cc = *c.cfg;
  if (lane >= cc.n_ctrl) return;
  const int k = cc.idx[lane];
  int32_t v = 0;
#pragma unroll
  for (int i = 0; i < SMB_STATS; i++) v = i == k ? stats[i] : v;
  const double range = cc.range[lane];
  float2 out;
  out.x = (float)(C.v[2 * SMB_STATS + lane] / range);
  out.y = (float)((double)v / range);
  ((float2 *)c.obs)[(size_t)row * cc.n_ctrl + lane] = out;
}
__device__ __forceinline__ void smb_ctrl_write_obs(const SmbCtrlNone &, const SmbCtrlArgs &, int, int, const int32_t *) {}

#ifdef PCGRL_SMB_CTRL_KERNELS  // (smb/pcgrl_k_smb_env.hip has them)
// pcgrl_smb_ctrl_queue: set_trgs replaces the whole queue (control_wrappers.py:167-168), so the set of named controls is
// stored, not added to.  One thread per env.
__global__ __launch_bounds__(256) void smb_ctrl_queue_kernel(const SmbCtrlQueueArgs a) {
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env >= a.n) return;
  if (a.mask && a.mask[env] == 0) return;
  SmbCtrlRec *R = a.rec + env;
  int32_t qmask = 0;
  for (int i = 0; i < a.n_named; i++) {
    const int j = a.named[i];
    const size_t at = (size_t)env * a.n_named + i;
    R->q[j][0] = a.lo[at];
    R->q[j][1] = a.hi[at];
    R->q[j][2] = a.obs[at];
    qmask |= 1 << j;
  }
  R->qmask = qmask;
  R->flag |= 1;
}

__global__ __launch_bounds__(256) void smb_ctrl_get_kernel(const SmbCtrlGetArgs a) {
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env >= a.n) return;
  const SmbCtrlRec *R = a.rec + env;
  for (int k = 0; k < SMB_STATS; k++) {
    if (a.active) {
      a.active[((size_t)env * SMB_STATS + k) * 2] = R->lo[k];
      a.active[((size_t)env * SMB_STATS + k) * 2 + 1] = R->hi[k];
    }
    if (a.shown) a.shown[(size_t)env * SMB_STATS + k] = R->obs[k];
    if (a.queued)
      for (int i = 0; i < 3; i++) a.queued[((size_t)env * SMB_STATS + k) * 3 + i] = R->q[k][i];
  }
  if (a.flags) {
    a.flags[(size_t)env * 2] = R->flag;
    a.flags[(size_t)env * 2 + 1] = R->qmask;
  }
}

// the control observation of the committed state; one thread per env and control
__global__ __launch_bounds__(256) void smb_ctrl_observe_kernel(const SmbCtrlObserveArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const SmbCtrlCfg &cc = *a.c.cfg;
  const int K = cc.n_ctrl;
  if (t >= a.n * K) return;
  const int env = t / K, j = t % K;
  const int32_t *stats = (const int32_t *)((const uint8_t *)a.stats + (size_t)env * a.stats_stride + a.stats_offset);
  const double range = cc.range[j];
  a.c.obs[(size_t)t * 2] = (float)(a.c.rec[env].obs[j] / range);
  a.c.obs[(size_t)t * 2 + 1] = (float)((double)stats[cc.idx[j]] / range);
}

__global__ __launch_bounds__(64) void smb_ctrl_resample_kernel(const SmbCtrlResampleArgs a) {
  const int j = threadIdx.x;
  if (j < a.n_ctrl) {
    a.cfg->rs_lo[j] = a.lo[j];
    a.cfg->rs_hi[j] = a.hi[j];
  }
  if (j == 0) {
    a.cfg->seed = a.seed;
    a.cfg->enable = a.enable;
  }
}
#endif  // PCGRL_SMB_CTRL_KERNELS

#endif  // PCGRL_KERNEL_TU

}  // namespace pcgrl
