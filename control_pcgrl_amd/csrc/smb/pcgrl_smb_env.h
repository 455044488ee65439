// smb/pcgrl_smb_env.h -- stepping Super Mario Bros environments on the device (include/pcgrl_amd_smb_env.h): what make_env(cfg)
// of the reference does for smb + narrow / turtle -- reset, representation update, statistics, reward, done, observation and the
// automatic reset.  DESIGN.md section 18 has the rules; tests/smb_env_rules.py is the same in plain Python.
//
// One 64-lane wave per env, the map as bytes in LDS (SmbLds of smb/pcgrl_smb.h), one launch per step and one per reset.
//   state     per env in HBM: the map (bytes, rows of `map_stride` = H * W rounded up to 16 so that it moves in 16-byte pieces),
//             an SmbEnvState record, the two PCG64 streams (RngState) and the evaluator's workspace slot.
//   step      load -> action -> statistics -> loss, reward, done -> latch the finished episode -> (auto_reset) draw the next map
//             -> observation -> state.  The observation depends on the map and the position only, so its stores are issued
//             BEFORE the search and drain under it; at an automatic reset they follow the new map's draw instead.
//   pieces    the rules of a step and of a reset stand once, as device functions (smb_env_bad_action, _update, _restat, _emit,
//             _latch, _inject, _reset_map, _commit_reset): the kernels below, the asynchronous ones (smb/pcgrl_smb_ready.h), the
//             rollout (smb/pcgrl_smb_rollout.h) and the state set (smb/pcgrl_smb_state.h) compose them, each in its own order.
//             DESIGN.md section 25 has the orders and the deliberate differences.
//   shortcuts both exact: (1) the written tile equals the old one -> the statistics stay (the reference's own rule,
//             pcgrl_env.py:314); (2) the tile changes but the cell's solidity (solid, brick, question, tube against the rest)
//             does not -> the play-through's level is the same, so only the five map statistics are rescanned and jumps,
//             jumps-dist, dist-win and sol-length keep their values.  A reset always searches.  `searches` counts them.
//   draw      as reset_from_rng of pcgrl_kernels2d.h: every lane replays the seven doubles of the problem stream and the turtle's
//             two; the H * W map draws are split over the lanes in runs of ceil(H * W / 64) cells with the LCG skip-ahead table.
//   obs       [oh][ow][8] bytes, a cell is one 8-byte one-hot word (byte 0 = outside the map, byte 1 + tile inside); all lanes
//             store two cells at a time as 16 bytes (8 bytes each when oh * ow is odd: an env's rows then start on 8 only).
//   errors    err[0] bit 0: an action outside the space (the env is left as it was: reward 0, not done, the same observation);
//             bit 1: a tile id above 6 in init_grids (read as empty).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../pcgrl_common.h"
#include "pcgrl_smb.h"
#include "pcgrl_smb_ctrl.h"

namespace pcgrl {

struct alignas(16) SmbEnvState {
  int32_t pos[2];
  int32_t n_step;     // narrow: updates since the reset (the scan counter)
  int32_t iteration, changes;
  int32_t searches;   // play-throughs run for this env since it was created
  int32_t ep_len;
  int32_t last_len;   // the last finished episode: length, count, return, final statistics
  int32_t stats[SMB_STATS];
  int32_t last_stats[SMB_STATS];
  int32_t last_count;
  int32_t iters_max;  // the most search iterations (both passes) one call spent on this env
  double last_loss, ep_return, last_return;
  int64_t iters_total;  // search iterations (both passes) spent on this env
};
static_assert(sizeof(SmbEnvState) == 144, "SmbEnvState layout");

struct SmbEnvArgs {
  int32_t h, w, rep, oh, ow, max_iterations, max_changes, power, n, map_stride;
  uint8_t *maps;       // [n][map_stride]
  SmbEnvState *st;     // [n]
  RngState *rng;       // [n]
  const JumpEntry *jump;  // [65]: entry l skips l * ceil(h * w / 64) draws, entry 64 skips h * w
  uint8_t *ws;
  int64_t ws_stride;
  int32_t *err;
  // per call
  const int32_t *actions;
  const uint8_t *mask, *init_grids;
  const int32_t *init_pos;  // [n][2]
  int32_t auto_reset;
  uint8_t *obs;
  float *reward;
  double *reward64;
  uint8_t *done;
  int32_t *stats_out;
  int32_t has_trg[SMB_STATS];
  double weight[SMB_STATS], trg_lo[SMB_STATS], trg_hi[SMB_STATS];
  SmbCtrlArgs ctrl;  // a controllable handle (smb/pcgrl_smb_ctrl.h): the per-env targets replace trg_lo / trg_hi
};

// what pcgrl_smb_env_get_state / get_last_episode gather; any pointer may be null
struct SmbEnvGather {
  int32_t n, h, w, map_stride;
  const uint8_t *maps;
  const SmbEnvState *st;
  uint8_t *grids;      // [n][h * w]
  int32_t *pos;        // [n][2]
  int32_t *counters;   // [n][4]: iteration, changes, n_step, searches
  int32_t *stats;      // [n][9]
  double *last_loss, *ep_return;
  int64_t *iters;      // [n][2]: total, max per call
  double *last_return;
  int32_t *last_len, *last_stats, *last_count;
};

enum SmbEnvKernel { SMB_ENV_RESET = 0, SMB_ENV_STEP = 1, SMB_ENV_OBSERVE = 2 };
hipError_t launch_smb_env(SmbEnvKernel k, const SmbEnvArgs &a, hipStream_t s);
hipError_t launch_smb_env_gather(const SmbEnvGather &g, hipStream_t s);

#ifdef PCGRL_KERNEL_TU
}  // namespace pcgrl
#include "../pcgrl_kernels2d.h"  // Pcg
namespace pcgrl {

__device__ __forceinline__ bool smb_tile_solid(int t) { return t == 1 || t == 3 || t == 4 || t == 6; }

// ControlWrapper.get_loss against the handle's static targets
__device__ __forceinline__ double smb_env_loss(const SmbEnvArgs &a, const int32_t *stats) {
  return smb_target_loss(a.has_trg, a.weight, a.trg_lo, a.trg_hi, stats);
}
// the same against the targets a controllable launch holds in LDS (SmbCtrlNone: the static ones above)
__device__ __forceinline__ double smb_env_loss(const SmbEnvArgs &a, const int32_t *stats, const SmbCtrlNone &) {
  return smb_env_loss(a, stats);
}
__device__ __forceinline__ double smb_env_loss(const SmbEnvArgs &a, const int32_t *stats, const SmbCtrlLds &C) {
  return smb_ctrl_loss(C, a.has_trg, a.weight, stats);
}

// envs/pcgrl_env.py:158-188: the next episode's map into L.map and its start into pos; lane 0 stores the advanced streams
__device__ inline void smb_env_draw(SmbLds &L, const SmbEnvArgs &a, int env, int lane, int *pos) {
  const int H = a.h, W = a.w, cells = H * W, cpl = (cells + 63) >> 6;
  Pcg rp, rr;
  rp.load(a.rng[env].prob);
  rr.load(a.rng[env].rep);
  double cdf[SMB_TILES], total = 0.0;
#pragma unroll
  for (int t = 0; t < SMB_TILES; t++) cdf[t] = rp.next_double();
#pragma unroll
  for (int t = 0; t < SMB_TILES; t++) total += cdf[t];
  double acc = 0.0;
#pragma unroll
  for (int t = 0; t < SMB_TILES; t++) {
    acc += cdf[t] / total;
    cdf[t] = acc;
  }
#pragma unroll
  for (int t = 0; t < SMB_TILES; t++) cdf[t] /= acc;
  pos[0] = pos[1] = 0;
  if (a.rep == PCGRL_REP_TURTLE) {  // turtle_rep.py:31-44, before the map
    pos[0] = (int)(rr.next_double() * (double)H);
    pos[1] = (int)(rr.next_double() * (double)W);
  }
  Pcg end = rr;
  end.jump(a.jump[64]);
  const int lo = lane * cpl, hi = min(lo + cpl, cells);
  if (lo < cells) {
    rr.jump(a.jump[lane]);
    for (int i = lo; i < hi; i++) {
      const double u = rr.next_double();
      int idx = 0;
#pragma unroll
      for (int t = 0; t < SMB_TILES; t++) idx += cdf[t] <= u ? 1 : 0;  // searchsorted(cdf, u, side='right')
      L.map[i] = (uint8_t)min(idx, SMB_TILES - 1);
    }
  }
  if (lane == 0) {
    end.store(a.rng[env].rep);
    rp.store(a.rng[env].prob);
  }
}

// the cropped one-hot observation of the map in L.map around pos (wrappers.py:407-437)
__device__ inline void smb_env_write_obs(const SmbLds &L, const SmbEnvArgs &a, int env, int lane, int p0, int p1) {
  if (!a.obs) return;
  const int H = a.h, W = a.w, OH = a.oh, OW = a.ow, n = OH * OW;
  uint8_t *base = a.obs + (size_t)env * n * 8;
  const int r0 = p0 - OH / 2, c0 = p1 - OW / 2;
  auto cell = [&](int i) -> uint64_t {
    const int r = r0 + i / OW, c = c0 + i % OW;
    const int ch = (r >= 0 && r < H && c >= 0 && c < W) ? 1 + (int)L.map[r * W + c] : 0;
    return 1ull << (8 * ch);
  };
  if ((n & 1) == 0) {
    for (int i = 2 * lane; i < n; i += 128) {
      const uint64_t v0 = cell(i), v1 = cell(i + 1);
      *(uint4 *)(base + (size_t)i * 8) = make_uint4((uint32_t)v0, (uint32_t)(v0 >> 32), (uint32_t)v1, (uint32_t)(v1 >> 32));
    }
  } else {
    for (int i = lane; i < n; i += 64) *(uint64_t *)(base + (size_t)i * 8) = cell(i);
  }
}

__device__ inline void smb_env_load_map(SmbLds &L, const SmbEnvArgs &a, int env, int lane) {
  const uint4 *src = (const uint4 *)(a.maps + (size_t)env * a.map_stride);
  for (int i = lane; i < a.map_stride / 16; i += 64) ((uint4 *)L.map)[i] = src[i];
}
__device__ inline void smb_env_store_map(const SmbLds &L, const SmbEnvArgs &a, int env, int lane) {
  uint4 *dst = (uint4 *)(a.maps + (size_t)env * a.map_stride);
  for (int i = lane; i < a.map_stride / 16; i += 64) dst[i] = ((const uint4 *)L.map)[i];
}

// the env's workspace slot: the search's nodes, then its heap
__device__ __forceinline__ uint2 *smb_env_nodes(const SmbEnvArgs &a, int env) {
  return (uint2 *)(a.ws + (size_t)env * a.ws_stride);
}
__device__ __forceinline__ uint32_t *smb_env_heap(const SmbEnvArgs &a, int env) {
  return (uint32_t *)(a.ws + (size_t)env * a.ws_stride + smb_nodes_per_pass(a.power) * 8);
}

// a fresh episode on the map in L.map: the search, the counters, last_loss (every lane holds the same S)
template <class CtrlLds>
__device__ inline void smb_env_begin(SmbLds &L, const SmbEnvArgs &a, int env, SmbEnvState &S, const int *pos, CtrlLds &C) {
  SmbResult r;
  smb_evaluate_level(L, a.h, a.w, a.power, smb_env_nodes(a, env), smb_env_heap(a, env), SmbPlayOut{nullptr, nullptr, 0, 0}, r);
#pragma unroll
  for (int k = 0; k < SMB_STATS; k++) S.stats[k] = r.stats[k];
  S.pos[0] = pos[0];
  S.pos[1] = pos[1];
  S.n_step = S.iteration = S.changes = S.ep_len = 0;
  S.searches++;
  S.iters_total += r.it1 + r.it2;
  S.iters_max = max(S.iters_max, r.it1 + r.it2);
  S.ep_return = 0.0;
  smb_ctrl_take(C, a.ctrl, env, threadIdx.x & 63);  // the queued or resampled targets, before the new level's loss
  S.last_loss = smb_env_loss(a, S.stats, C);
}

// ---- The pieces of a transition.  Every kernel that steps or resets an env -- smb_env_step_kernel and smb_env_reset_kernel below,
// smb_ready_step_kernel and smb_ready_reset_kernel (smb/pcgrl_smb_ready.h), smb_env_rollout_kernel (smb/pcgrl_smb_rollout.h) and
// smb_state_set_kernel (smb/pcgrl_smb_state.h) -- composes them in its own order; the rules stand here alone.  Every lane calls
// them with the same S; `row` is the row of the per-step outputs (env, or k * n + env in a rollout).

// the four per-row outputs of a step, by lane 0
__device__ __forceinline__ void smb_env_write_row(const SmbEnvArgs &a, size_t row, int lane, double reward, bool done,
                                                  const int32_t *stats) {
  if (lane != 0) return;
  if (a.reward) a.reward[row] = (float)reward;
  if (a.reward64) a.reward64[row] = reward;
  if (a.done) a.done[row] = done ? 1 : 0;
  if (a.stats_out)
    for (int k = 0; k < SMB_STATS; k++) a.stats_out[row * SMB_STATS + k] = stats[k];
}

// an action outside the space (pcgrl_step's rule): error bit 0, reward 0, not done, the same statistics, the env as it was.
// The observation (and a ready step's status) is the caller's.
__device__ __forceinline__ bool smb_env_bad_action(const SmbEnvArgs &a, int act, int n_act, size_t row, int lane,
                                                   const SmbEnvState &S) {
  if (act >= 0 && act < n_act) return false;
  if (lane == 0) atomicOr(a.err, 1);
  smb_env_write_row(a, row, lane, 0.0, false, S.stats);
  return true;
}

// what the representation's update leaves beside the counters in S
struct SmbEnvEdit {
  int pos[2];             // the position after the update (committed by smb_env_emit)
  bool changed, resolid;  // the written tile differs from the old one; the cell's solidity differs
  bool done;
};

// the representation's update (narrow_rep.py:89-102, turtle_rep.py:87-107) on the map in L.map, the counters and done
// (pcgrl_env.py:307-309).  A written tile is stored by lane 0 between two barriers.
__device__ __forceinline__ SmbEnvEdit smb_env_update(SmbLds &L, const SmbEnvArgs &a, int act, int lane, SmbEnvState &S) {
  const int H = a.h, W = a.w;
  SmbEnvEdit e = {{S.pos[0], S.pos[1]}, false, false, false};
  int tile = -1;
  if (a.rep == PCGRL_REP_NARROW) {
    tile = act;
  } else if (act < 4) {
    const int dr = act == 0 ? -1 : (act == 1 ? 1 : 0), dc = act == 2 ? -1 : (act == 3 ? 1 : 0);
    e.pos[0] = min(max(e.pos[0] + dr, 0), H - 1);
    e.pos[1] = min(max(e.pos[1] + dc, 0), W - 1);
  } else {
    tile = act - 4;
  }
  if (tile >= 0) {
    const int idx = e.pos[0] * W + e.pos[1];
    const int old = L.map[idx];
    e.changed = old != tile;
    e.resolid = smb_tile_solid(old) != smb_tile_solid(tile);
    __syncthreads();
    if (lane == 0) L.map[idx] = (uint8_t)tile;
    __syncthreads();
  }
  if (a.rep == PCGRL_REP_NARROW) {  // the position the NEXT update writes: cell n_step mod cells, then n_step + 1
    const int c = S.n_step % (H * W);
    e.pos[0] = c / W;
    e.pos[1] = c % W;
    S.n_step++;
  }
  S.iteration++;
  S.changes += e.changed ? 1 : 0;
  S.ep_len++;
  e.done = S.iteration > a.max_iterations;
  if (a.max_changes >= 0) e.done = e.done || S.changes > a.max_changes;
  return e;
}

// the statistics of the edited map in L.map by the two exact shortcuts, the search run to its end: the five map statistics, and
// the play-through's four where the edit changed the level's solidity
__device__ __forceinline__ void smb_env_restat(SmbLds &L, const SmbEnvArgs &a, int env, bool resolid, SmbEnvState &S) {
  SmbResult r;
  smb_scan_level(L, a.h, a.w, r);
#pragma unroll
  for (int k = 0; k < 5; k++) S.stats[k] = r.stats[k];
  if (!resolid) return;
  smb_play_level(L, a.h, a.w, a.power, smb_env_nodes(a, env), smb_env_heap(a, env), SmbPlayOut{nullptr, nullptr, 0, 0}, r);
#pragma unroll
  for (int k = 5; k < SMB_STATS; k++) S.stats[k] = r.stats[k];
  S.searches++;
  S.iters_total += r.it1 + r.it2;
  S.iters_max = max(S.iters_max, r.it1 + r.it2);
}

// loss and reward (control_wrappers.py:227-229) of the step that left S.stats, the new position, and the step's output row
template <class CtrlLds>
__device__ __forceinline__ void smb_env_emit(const SmbEnvArgs &a, size_t row, int lane, const SmbEnvEdit &e, SmbEnvState &S,
                                             const CtrlLds &C) {
  const double loss = smb_env_loss(a, S.stats, C);
  const double reward = loss - S.last_loss;
  S.last_loss = loss;
  S.ep_return += reward;
  S.pos[0] = e.pos[0];
  S.pos[1] = e.pos[1];
  smb_env_write_row(a, row, lane, reward, e.done, S.stats);
}

// the latch of the finished episode
__device__ __forceinline__ void smb_env_latch(SmbEnvState &S) {
  S.last_return = S.ep_return;
  S.last_len = S.ep_len;
  S.last_count++;
#pragma unroll
  for (int k = 0; k < SMB_STATS; k++) S.last_stats[k] = S.stats[k];
}

// a caller's map into L.map: the padding of the stored row zeroed, the tile rule, error bit 1
__device__ __forceinline__ void smb_env_clear_padding(SmbLds &L, const SmbEnvArgs &a, int lane) {
  for (int i = a.h * a.w + lane; i < a.map_stride; i += 64) L.map[i] = 0;
}
__device__ __forceinline__ void smb_env_inject(SmbLds &L, const SmbEnvArgs &a, int env, int lane) {
  const int cells = a.h * a.w;
  smb_env_clear_padding(L, a, lane);
  const uint8_t *g = a.init_grids + (size_t)env * cells;
  bool bad = false;
  for (int i = lane; i < cells; i += 64) L.map[i] = smb_tile(g[i], bad);
  if (__any(bad) && lane == 0) atomicOr(a.err, 2);
}

// a reset's map into L.map and its start into pos: injected (it draws nothing, as pcgrl_reset does; init_pos clamped) or drawn
__device__ __forceinline__ void smb_env_reset_map(SmbLds &L, const SmbEnvArgs &a, int env, int lane, int *pos) {
  if (!a.init_grids) {
    smb_env_clear_padding(L, a, lane);
    smb_env_draw(L, a, env, lane, pos);
    return;
  }
  smb_env_inject(L, a, env, lane);
  pos[0] = pos[1] = 0;
  if (a.init_pos && a.rep == PCGRL_REP_TURTLE) {
    pos[0] = min(max(a.init_pos[(size_t)env * 2], 0), a.h - 1);
    pos[1] = min(max(a.init_pos[(size_t)env * 2 + 1], 0), a.w - 1);
  }
}

// What a reset writes back (lane 0): only the fields it owns -- the last finished episode stays where it is -- and the search's
// (searches, last_loss, the statistics) only when the search is over: pending statistics keep the old ones until then.
__device__ __forceinline__ void smb_env_commit_reset(SmbEnvState *P, const SmbEnvState &S, bool finished) {
  P->pos[0] = S.pos[0];
  P->pos[1] = S.pos[1];
  P->n_step = P->iteration = P->changes = P->ep_len = 0;
  P->iters_total = S.iters_total;
  P->iters_max = S.iters_max;
  P->ep_return = 0.0;
  if (!finished) return;
  P->searches = S.searches;
  P->last_loss = S.last_loss;
#pragma unroll
  for (int k = 0; k < SMB_STATS; k++) P->stats[k] = S.stats[k];
}


#ifndef PCGRL_SMB_ENV_DEVICE_ONLY  // (smb/pcgrl_k_smb_ready.hip composes the pieces above without a second set of kernels)
template <bool CTRL>
__global__ __launch_bounds__(64) void smb_env_reset_kernel(const SmbEnvArgs a) {
  __shared__ SmbLds L;
  __shared__ typename SmbCtrlLdsOf<CTRL>::type C;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= a.n) return;
  const bool active = !a.mask || a.mask[env] != 0;
  SmbEnvState *P = a.st + env;
  smb_ctrl_load(C, a.ctrl, env, lane);
  SmbEnvState S;  // what smb_env_begin reads and writes; the last finished episode stays where it is
  S.searches = P->searches;
  S.iters_total = P->iters_total;
  S.iters_max = P->iters_max;
  int pos[2] = {P->pos[0], P->pos[1]};
  if (!active) {  // the env stays as it is; its observation is written all the same
    smb_env_load_map(L, a, env, lane);
    __syncthreads();
    smb_env_write_obs(L, a, env, lane, pos[0], pos[1]);
    if constexpr (CTRL) smb_ctrl_write_obs(C, a.ctrl, env, lane, P->stats);
    return;
  }
  smb_env_reset_map(L, a, env, lane, pos);
  __syncthreads();
  smb_env_write_obs(L, a, env, lane, pos[0], pos[1]);
  smb_env_store_map(L, a, env, lane);
  smb_env_begin(L, a, env, S, pos, C);
  smb_ctrl_write_obs(C, a.ctrl, env, lane, S.stats);
  if (lane == 0) smb_env_commit_reset(P, S, true);
}

__global__ __launch_bounds__(64) void smb_env_observe_kernel(const SmbEnvArgs a) {
  __shared__ SmbLds L;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= a.n) return;
  smb_env_load_map(L, a, env, lane);
  __syncthreads();
  smb_env_write_obs(L, a, env, lane, a.st[env].pos[0], a.st[env].pos[1]);
}

template <bool CTRL>
__global__ __launch_bounds__(64) void smb_env_step_kernel(const SmbEnvArgs a) {
  __shared__ SmbLds L;
  __shared__ typename SmbCtrlLdsOf<CTRL>::type C;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= a.n) return;
  smb_env_load_map(L, a, env, lane);
  SmbEnvState S = a.st[env];
  smb_ctrl_load(C, a.ctrl, env, lane);
  const int act = a.actions[env];
  __syncthreads();
  if (smb_env_bad_action(a, act, a.rep == PCGRL_REP_NARROW ? SMB_TILES : 4 + SMB_TILES, env, lane, S)) {
    smb_env_write_obs(L, a, env, lane, S.pos[0], S.pos[1]);
    smb_ctrl_write_obs(C, a.ctrl, env, lane, S.stats);
    return;
  }
  SmbEnvEdit e = smb_env_update(L, a, act, lane, S);
  const bool renew = e.done && a.auto_reset != 0;
  if (!renew) smb_env_write_obs(L, a, env, lane, e.pos[0], e.pos[1]);  // drains under the search
  if (e.changed) {
    smb_env_store_map(L, a, env, lane);  // before the search: a synchronous step always ends in this launch
    smb_env_restat(L, a, env, e.resolid, S);
  }
  smb_env_emit(a, env, lane, e, S, C);
  if (e.done) smb_env_latch(S);
  if (renew) {  // the next episode inside the same launch: the observation returned is its first
    __syncthreads();
    smb_env_draw(L, a, env, lane, e.pos);
    __syncthreads();
    smb_env_write_obs(L, a, env, lane, e.pos[0], e.pos[1]);
    smb_env_store_map(L, a, env, lane);
    smb_env_begin(L, a, env, S, e.pos, C);
  }
  smb_ctrl_write_obs(C, a.ctrl, env, lane, S.stats);  // the new episode's, where the step began one
  if (lane == 0) a.st[env] = S;
}

__global__ __launch_bounds__(64) void smb_env_gather_kernel(const SmbEnvGather g) {
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= g.n) return;
  const int cells = g.h * g.w;
  if (g.grids)
    for (int i = lane; i < cells; i += 64) g.grids[(size_t)env * cells + i] = g.maps[(size_t)env * g.map_stride + i];
  if (lane != 0) return;
  const SmbEnvState &S = g.st[env];
  if (g.pos) g.pos[env * 2] = S.pos[0], g.pos[env * 2 + 1] = S.pos[1];
  if (g.counters) {
    int32_t *c = g.counters + (size_t)env * 4;
    c[0] = S.iteration, c[1] = S.changes, c[2] = S.n_step, c[3] = S.searches;
  }
  if (g.last_loss) g.last_loss[env] = S.last_loss;
  if (g.ep_return) g.ep_return[env] = S.ep_return;
  if (g.iters) g.iters[env * 2] = S.iters_total, g.iters[env * 2 + 1] = S.iters_max;
  if (g.last_return) g.last_return[env] = S.last_return;
  if (g.last_len) g.last_len[env] = S.last_len;
  if (g.last_count) g.last_count[env] = S.last_count;
  for (int k = 0; k < SMB_STATS; k++) {
    if (g.stats) g.stats[(size_t)env * SMB_STATS + k] = S.stats[k];
    if (g.last_stats) g.last_stats[(size_t)env * SMB_STATS + k] = S.last_stats[k];
  }
}

#endif  // PCGRL_SMB_ENV_DEVICE_ONLY

#endif  // PCGRL_KERNEL_TU

}  // namespace pcgrl
