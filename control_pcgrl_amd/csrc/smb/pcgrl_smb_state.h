// smb/pcgrl_smb_state.h -- checkpoint and restore of Super Mario Bros environments (include/pcgrl_amd_smb_state.h): the image of
// pcgrl_smb_state_export / _import, the portable pcgrl_smb_state_set and the RNG streams in and out.  DESIGN.md section 20 has
// the layout and the restart rule; tests/smb_state_rules.py is the same in plain Python.
//
// One 64-lane wave per env, one launch per call, as the stepping kernels.
//   image     a 256-byte header, then four sections contiguous over the envs, each a multiple of 16 bytes per env but the last:
//             the stored map rows [n][map_stride], the SmbEnvState records [n][144], the streams [n][10] uint64 in the layout of
//             pcgrl_get_rng_state (words 8 and 9, the kept 32-bit half, are zero: an SMB env draws doubles only) and
//             [n][2] int32 = ready mode, pending action.  Sections, not records: a record would be map_stride + 232 bytes, a
//             multiple of 8 only, and the 16-byte moves of the map rows would be lost.
//   export    copies; the header comes from pinned host memory the library owns, by the lanes of block 0.  A busy env's
//             iters_total goes out WITHOUT the iterations its parked search has spent so far: that search is not in the image
//             and runs again from iteration 0 after an import, which counts them a second time.
//   import    env j takes row index[j] of the image.  A busy row's search starts over: the import writes "parked after 0
//             iterations" -- smb_search_start's nodes[0], heap[0] and loop words, and a zeroed visited set -- so the stepping
//             kernels resume it as they resume any parked search.
//   set       the map, position, counters and return from the caller; the nine statistics and last_loss by the level's
//             evaluation, under the budget where one is set (unfinished -> pending statistics, as a reset leaves them).
//   controls  the image of a controllable env (smb/pcgrl_smb_ctrl.h) has a fifth section, the SmbCtrlRec records [n][448], on the
//             next 16-byte boundary: active and queued targets, the queue set and the flag word with the draw counter.  The
//             resampling switch, seed and bounds are run-time state and are not in the image.  Without controls there is no
//             such section and the image is what it was.
//   errors    err[0] bit 1: a tile id above 6 in pcgrl_smb_state_set's maps (read as empty); bit 2: an index entry outside
//             0..n-1 (the env is left as it was).
#pragma once
#include <cstddef>

#include "pcgrl_smb_ready.h"

namespace pcgrl {

constexpr int SMB_STATE_HDR_BYTES = 256;
constexpr int SMB_STATE_RNG_WORDS = 10;
static_assert(offsetof(SmbEnvState, iters_total) == 136 && sizeof(SmbEnvState) == 9 * 16, "the export patches the last 16 bytes");
static_assert(sizeof(RngState) == 64, "RngState layout");

// where the sections of an image of n envs start
struct SmbStateLayout {
  int64_t maps, st, rng, mode, total, ctrl;
};
__host__ __device__ inline SmbStateLayout smb_state_layout(int n, int map_stride, bool ctrl = false) {
  SmbStateLayout l;
  l.maps = SMB_STATE_HDR_BYTES;
  l.st = l.maps + (int64_t)n * map_stride;
  l.rng = l.st + (int64_t)n * (int64_t)sizeof(SmbEnvState);
  l.mode = l.rng + (int64_t)n * SMB_STATE_RNG_WORDS * 8;
  l.total = l.mode + (int64_t)n * 8;
  l.ctrl = (l.total + 15) & ~(int64_t)15;
  if (ctrl) l.total = l.ctrl + (int64_t)n * (int64_t)sizeof(SmbCtrlRec);
  return l;
}

struct SmbStateArgs {
  SmbReadyArgs r;      // r.park null: no budget was ever set; r.budget 0: synchronous stepping
  const uint8_t *hdr;  // export: the pinned header
  uint8_t *image;      // export writes it, import reads it
  const int32_t *index;
  // pcgrl_smb_state_set (the mask and the maps are r.e.mask and r.e.init_grids)
  const int32_t *pos, *counters;
  const double *ep_return;
  // the streams
  uint64_t *rng_out;
  const uint64_t *rng_in;
};

enum SmbStateKernel { SMB_STATE_EXPORT = 0, SMB_STATE_IMPORT = 1, SMB_STATE_SET = 2, SMB_STATE_RNG = 3 };
hipError_t launch_smb_state(SmbStateKernel k, const SmbStateArgs &a, hipStream_t s);

#ifdef PCGRL_KERNEL_TU

__global__ __launch_bounds__(64) void smb_state_export_kernel(const SmbStateArgs sa) {
  const SmbEnvArgs &a = sa.r.e;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= a.n) return;
  const SmbStateLayout l = smb_state_layout(a.n, a.map_stride, a.ctrl.rec != nullptr);
  if (env == 0 && lane < SMB_STATE_HDR_BYTES / 16) ((uint4 *)sa.image)[lane] = ((const uint4 *)sa.hdr)[lane];
  const uint4 *src = (const uint4 *)(a.maps + (size_t)env * a.map_stride);
  uint4 *dst = (uint4 *)(sa.image + l.maps + (size_t)env * a.map_stride);
  for (int i = lane; i < a.map_stride / 16; i += 64) dst[i] = src[i];
  int mode = SMB_READY_IDLE, action = 0, in_flight = 0;
  if (sa.r.park) {
    const SmbPark *P = sa.r.park + env;
    mode = P->mode;
    if (mode == SMB_READY_PENDING_STEP) action = P->action;
    if (mode != SMB_READY_IDLE) in_flight = P->it + (P->pass == 1 ? P->it1 : 0);
  }
  if (lane < 9) {
    uint4 v = ((const uint4 *)(a.st + env))[lane];
    if (lane == 8) {  // last_return, iters_total
      const uint64_t t = (((uint64_t)v.w << 32) | v.z) - (uint64_t)in_flight;
      v.z = (uint32_t)t;
      v.w = (uint32_t)(t >> 32);
    }
    ((uint4 *)(sa.image + l.st))[(size_t)env * 9 + lane] = v;
  }
  if (lane < SMB_STATE_RNG_WORDS) {
    const uint64_t *r = (const uint64_t *)(a.rng + env);
    ((uint64_t *)(sa.image + l.rng))[(size_t)env * SMB_STATE_RNG_WORDS + lane] = lane < 8 ? r[lane] : 0ull;
  }
  if (lane == 0) ((int2 *)(sa.image + l.mode))[env] = make_int2(mode, action);
  if (a.ctrl.rec && lane < (int)(sizeof(SmbCtrlRec) / 16))
    ((uint4 *)(sa.image + l.ctrl))[(size_t)env * (sizeof(SmbCtrlRec) / 16) + lane] = ((const uint4 *)(a.ctrl.rec + env))[lane];
}

__global__ __launch_bounds__(64) void smb_state_import_kernel(const SmbStateArgs sa) {
  const SmbEnvArgs &a = sa.r.e;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= a.n) return;
  if (a.mask && a.mask[env] == 0) return;  // the env stays as it is, parked search included
  const int row = sa.index ? sa.index[env] : env;
  if (row < 0 || row >= a.n) {
    if (lane == 0) atomicOr(a.err, 4);
    return;
  }
  const SmbStateLayout l = smb_state_layout(a.n, a.map_stride, a.ctrl.rec != nullptr);
  const uint4 *src = (const uint4 *)(sa.image + l.maps + (size_t)row * a.map_stride);
  uint4 *dst = (uint4 *)(a.maps + (size_t)env * a.map_stride);
  for (int i = lane; i < a.map_stride / 16; i += 64) dst[i] = src[i];
  if (lane < 9) ((uint4 *)(a.st + env))[lane] = ((const uint4 *)(sa.image + l.st))[(size_t)row * 9 + lane];
  if (lane < 8) ((uint64_t *)(a.rng + env))[lane] = ((const uint64_t *)(sa.image + l.rng))[(size_t)row * SMB_STATE_RNG_WORDS + lane];
  if (a.ctrl.rec && lane < (int)(sizeof(SmbCtrlRec) / 16))
    ((uint4 *)(a.ctrl.rec + env))[lane] = ((const uint4 *)(sa.image + l.ctrl))[(size_t)row * (sizeof(SmbCtrlRec) / 16) + lane];
  if (!sa.r.park) return;  // (the host has refused a busy row for an env without a budget)
  int2 m = ((const int2 *)(sa.image + l.mode))[row];
  if (m.x != SMB_READY_PENDING_STEP && m.x != SMB_READY_PENDING_STATS) m = make_int2(SMB_READY_IDLE, 0);
  SmbPark *P = sa.r.park + env;
  if (lane == 0) {
    P->mode = m.x;
    P->action = m.y;
  }
  if (m.x == SMB_READY_IDLE) return;  // whatever was parked here is abandoned, as a masked reset abandons it
  // the row's search, parked after 0 iterations: a zeroed visited set and pass 1 as smb_play_budgeted starts it
  for (int i = lane; i < SMB_SEEN_WORDS; i += 64) P->seen[i] = 0;
  if (lane == 0) {
    P->pass = 0, P->it1 = 0;
    smb_search_start(smb_env_nodes(a, env), smb_env_heap(a, env), a.h, a.w, true, P->it, P->nn, P->hn, P->best, P->best_x,
                     P->best_depth);
  }
}

template <bool CTRL>
__global__ __launch_bounds__(64) void smb_state_set_kernel(const SmbStateArgs sa) {
  __shared__ SmbLds L;
  __shared__ typename SmbCtrlLdsOf<CTRL>::type C;
  const SmbEnvArgs &a = sa.r.e;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= a.n) return;
  if (a.mask && a.mask[env] == 0) return;
  smb_ctrl_load(C, a.ctrl, env, lane);  // the active targets: setting a state is no reset and takes nothing from the queue
  const int H = a.h, W = a.w;
  smb_env_inject(L, a, env, lane);
  __syncthreads();
  smb_env_store_map(L, a, env, lane);
  SmbEnvState *Q = a.st + env;
  // (only the fields the call writes are touched, as the reset kernels do: the last finished episode stays where it is)
  int p0 = 0, p1 = 0;
  if (sa.pos) {
    p0 = min(max(sa.pos[(size_t)env * 2], 0), H - 1);
    p1 = min(max(sa.pos[(size_t)env * 2 + 1], 0), W - 1);
  }
  const int32_t *c = sa.counters ? sa.counters + (size_t)env * 4 : nullptr;
  const int iteration = c ? c[0] : 0, changes = c ? c[1] : 0, n_step = c ? c[2] : 0;
  int searches = c ? c[3] : 0;
  const double ep_return = sa.ep_return ? sa.ep_return[env] : 0.0;
  uint2 *nodes = smb_env_nodes(a, env);
  uint32_t *heap = smb_env_heap(a, env);
  SmbResult r;
  bool finished = true;
  int spent;
  if (sa.r.budget > 0) {  // whatever was in flight is abandoned: a fresh search, under the budget
    int left = sa.r.budget;
    smb_scan_level(L, H, W, r);
    finished = smb_play_budgeted(L, H, W, a.power, nodes, heap, sa.r.park + env, false, left, r);
    spent = sa.r.budget - left;
    // the launch that ends pending statistics counts the search: `searches` then comes out as the caller gave it
    if (!finished) searches--;
    if (lane == 0) sa.r.park[env].mode = finished ? SMB_READY_IDLE : SMB_READY_PENDING_STATS;
  } else {
    const SmbPlayOut out = {nullptr, nullptr, 0, 0};
    smb_evaluate_level(L, H, W, a.power, nodes, heap, out, r);
    spent = r.it1 + r.it2;
    if (lane == 0 && sa.r.park) sa.r.park[env].mode = SMB_READY_IDLE;
  }
  if constexpr (CTRL) smb_ctrl_write_obs(C, a.ctrl, env, lane, finished ? r.stats : Q->stats);
  if (lane != 0) return;
  Q->pos[0] = p0;
  Q->pos[1] = p1;
  Q->iteration = iteration;
  Q->changes = changes;
  Q->n_step = n_step;
  Q->searches = searches;
  Q->ep_len = iteration;  // both count the steps since the episode began
  Q->ep_return = ep_return;
  Q->iters_total += spent;
  Q->iters_max = max(Q->iters_max, spent);
  if (finished) {  // pending statistics keep the old ones until the search is over
#pragma unroll
    for (int k = 0; k < SMB_STATS; k++) Q->stats[k] = r.stats[k];
    Q->last_loss = smb_env_loss(a, r.stats, C);
  }
}

// both streams out (rng_out) or in (rng_in, for the envs of the mask), one lane per word
__global__ __launch_bounds__(64) void smb_state_rng_kernel(const SmbStateArgs sa) {
  const SmbEnvArgs &a = sa.r.e;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= a.n || lane >= SMB_STATE_RNG_WORDS) return;
  uint64_t *r = (uint64_t *)(a.rng + env);
  if (sa.rng_out) sa.rng_out[(size_t)env * SMB_STATE_RNG_WORDS + lane] = lane < 8 ? r[lane] : 0ull;
  if (sa.rng_in && lane < 8 && (!a.mask || a.mask[env] != 0)) r[lane] = sa.rng_in[(size_t)env * SMB_STATE_RNG_WORDS + lane];
}

#endif  // PCGRL_KERNEL_TU

}  // namespace pcgrl
