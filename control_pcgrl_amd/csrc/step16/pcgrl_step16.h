// pcgrl_step16.h -- the binary 16x16 step (narrow / turtle, 32x32 observation window, plain mode) as a kernel of its own.
//
// pcgrl_k_step16.hip holds pcgrl::step16_kernel: the same two specialised waves per env quadruple as step_kernel
// (pcgrl_kernels2d.h) and the same state layout, with
//   * the wave's role decided first and one batch of loads per role in front of the workgroup barrier (step_kernel reads
//     flags / last_loss / ep_return / stats[] behind it: a second dependent memory round trip on every simulate wave),
//   * path sweeps that run every trip without the per-level bookkeeping and derive length, last level and visited set from
//     the frontiers of the group's last live trip (sweep16),
//   * the env record read and written back with 16-byte accesses,
//   * an observation encoder of its own: the chunks of the rows outside the map stored from registers first, the map rows
//     through LDS behind them.  Launches of up to 8 192 envs take encode_obs16_regs (six unconditional border stores per lane
//     off one scalar base, the map part of a row built in registers and written to LDS as dwords), larger ones encode_obs16
//     (conditional border trips, byte scatter), which the write-bound launches measured faster with.
// The host routes a step launch here when step16_applies() holds; every other launch takes launch_binary32 as before.
#pragma once
#include <hip/hip_runtime.h>

#include "../pcgrl_common.h"

namespace pcgrl {

// The launches step16_kernel is written for.  `plain`: neither per-env targets nor float64 rewards were asked for (the
// controllable-mode variant of step_kernel writes them; this kernel does not).
inline bool step16_applies(const Params &p, int lpe) {
  const pcgrl_config &c = p.cfg;
  const bool plain = p.trg == nullptr && p.reward64 == nullptr;
  return c.problem == PCGRL_PROB_BINARY && lpe == 16 && c.dims[0] == 16 && c.dims[1] == 16 &&
         (c.representation == PCGRL_REP_NARROW || c.representation == PCGRL_REP_TURTLE) && c.obs_window[0] == 32 &&
         c.obs_window[1] == 32 && p.obs != nullptr && !p.no_fast && !p.update_only && !p.ext && c.n_ctrl == 0 && !p.spread &&
         !p.sk_budget && !p.obs_codes && plain;
}

// lds: LDS bytes of one (simulate, observe) wave pair, as for launch_binary32
hipError_t launch_step16(const Params &p, size_t lds, hipStream_t s);

}  // namespace pcgrl
