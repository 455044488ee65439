// smb/pcgrl_smb_ready.h -- asynchronous stepping of Super Mario Bros environments (include/pcgrl_amd_smb_ready.h): the step and
// reset kernels of smb/pcgrl_smb_env.h with a budgeted, resumable A* play-through.  DESIGN.md section 19 has the launch rules;
// tests/smb_ready_rules.py is the same in plain Python.
//
// One 64-lane wave per env, as the synchronous kernels; a launch gives every env `budget` search iterations.
//   search    smb_play_budgeted runs smb_search_iteration of smb/pcgrl_smb.h -- the loop body smb_search itself runs -- on lane 0
//             until the search is over (won, it == power, open list empty) or the launch's iterations are spent.  Pass 2 starts
//             in the same launch with what is left.  A search whose last iteration spends the budget is over.
//   step      the step and reset kernels compose the transition's pieces of smb/pcgrl_smb_env.h as the synchronous kernels do,
//             but for the search under the budget, the map stored only once the search is over, and the early observation
//             also written where a renewing step's search may park (DESIGN.md section 25 lists the differences).
//   stays     the nodes and the heap are in the env's workspace slot in HBM already; while a search is parked the slot is not
//             scratch: nothing but the resumed search touches it.
//   parks     SmbPark, one per env, allocated by the library: the env's mode and pending action, the loop's words (pass, it, nn,
//             hn, best, best_x, best_depth, it1) and the visited bit set of the LDS (SMB_SEEN_WORDS words).  Only an env that
//             parks stores the loop's words and the set, only an env that resumes loads them; an env that finishes within its
//             launch reads the mode word and nothing else.
//   resume    the committed map is loaded, a pending step's edit is replayed in LDS from the parked action, and smb_scan_level
//             rebuilds the column masks and the five map statistics; nothing of the step in flight is stored before its search
//             ends, so the committed state (map, SmbEnvState) is the one before the step.
//   identity  a park record carries no copy of its map.  A busy env takes no action, so three calls alone can change a map under
//             a parked search, and each of them puts the park record right in the same launch: a reset and
//             pcgrl_smb_state_set (smb/pcgrl_smb_state.h) abandon the search and start the new map's, and
//             pcgrl_smb_state_import writes the record with the map -- idle, or the imported row's search "parked after 0
//             iterations" (smb_search_start), the start of a search of the map it has just stored.  The envs outside their
//             masks keep both.
//   dirty     a search starts by writing nodes[0], heap[0] and a zeroed visited set; mode is written by every reset: neither a
//             dirty workspace nor a dirty park record of a reset env matters.
#pragma once
#include "pcgrl_smb_env.h"

namespace pcgrl {

enum SmbReadyMode { SMB_READY_IDLE = 0, SMB_READY_PENDING_STEP = 1, SMB_READY_PENDING_STATS = 2 };

struct alignas(16) SmbPark {
  int32_t mode;    // SmbReadyMode
  int32_t action;  // the action a pending step consumed
  int32_t pass, it, nn, hn;
  uint32_t best;
  int32_t best_x, best_depth, it1;
  int32_t pad[2];
  uint32_t seen[SMB_SEEN_WORDS];
};
static_assert(sizeof(SmbPark) == 48 + SMB_SEEN_WORDS * 4 && sizeof(SmbPark) % 16 == 0, "SmbPark layout");

struct SmbReadyArgs {
  SmbEnvArgs e;
  SmbPark *park;    // [n]
  int32_t budget;   // search iterations per env and launch, >= 1
  uint8_t *status;  // [n]: PCGRL_ENV_EMITTED | PCGRL_ENV_BUSY (step only)
};

hipError_t launch_smb_ready_step(const SmbReadyArgs &a, hipStream_t s);
hipError_t launch_smb_ready_reset(const SmbReadyArgs &a, hipStream_t s);
hipError_t launch_smb_ready_busy(const SmbPark *park, int n, uint8_t *busy, hipStream_t s);

#ifdef PCGRL_KERNEL_TU

// The play half of a level's evaluation under a budget: `left` iterations may still run in this launch (it comes back with what
// the search left over).  resume: continue the search parked in P, else start one.  True when the search is over: r.stats[5..8]
// and the play record are then set as smb_play_level sets them.  False: the search is parked in P (the loop's words and the
// visited set; the caller sets mode and action).  Every lane returns with the same values.
__device__ inline bool smb_play_budgeted(SmbLds &L, int H, int W, int power, uint2 *nodes, uint32_t *heap, SmbPark *P, bool resume,
                                         int &left, SmbResult &r) {
  const int lane = threadIdx.x & 63;
  const int LW = W + 6, ex = W + 4;
  int pass = 0, it, nn, hn, best_x, best_depth, it1 = 0;
  uint32_t best;
  if (resume) {
    pass = P->pass, it = P->it, nn = P->nn, hn = P->hn, best = P->best, best_x = P->best_x, best_depth = P->best_depth;
    it1 = P->it1;
    for (int i = lane; i < SMB_SEEN_WORDS; i += 64) L.seen[i] = P->seen[i];
  } else {
    for (int i = lane; i < SMB_SEEN_WORDS; i += 64) L.seen[i] = 0;
    smb_search_start(nodes, heap, H, W, lane == 0, it, nn, hn, best, best_x, best_depth);
  }
  __syncthreads();
  int won = 0;
  bool over;
  for (;;) {
    if (lane == 0) {
      const int balance = pass == 0 ? 1 : 0;
      while (it < power && hn > 0 && left > 0) {
        it++;
        left--;
        if (smb_search_iteration(L.col, L.seen, nodes, heap, H, LW, ex, balance, nn, hn, best, best_x, best_depth)) {
          won = 1;
          break;
        }
      }
    }
    won = __shfl(won, 0, 64);
    it = __shfl(it, 0, 64);
    hn = __shfl(hn, 0, 64);
    left = __shfl(left, 0, 64);
    __syncthreads();
    over = won || it >= power || hn <= 0;
    if (!over || won || pass == 1) break;
    // pass 1 (balance 1) ended without a win: pass 2 (balance 0) starts from scratch, in this launch when iterations are left
    it1 = it;
    pass = 1;
    for (int i = lane; i < SMB_SEEN_WORDS; i += 64) L.seen[i] = 0;
    smb_search_start(nodes, heap, H, W, lane == 0, it, nn, hn, best, best_x, best_depth);
    __syncthreads();
    over = false;
    if (left <= 0) break;
  }
  if (!over) {
    for (int i = lane; i < SMB_SEEN_WORDS; i += 64) P->seen[i] = L.seen[i];
    if (lane == 0) {
      P->pass = pass, P->it = it, P->nn = nn, P->hn = hn, P->best = best, P->best_x = best_x, P->best_depth = best_depth;
      P->it1 = it1;
    }
    return false;
  }
  smb_play_result(W, nodes, best, won, pass == 0 ? it : it1, pass == 0 ? 0 : it, SmbPlayOut{nullptr, nullptr, 0, 0}, r);
  return true;
}

// the search iterations this launch spent on the env: the counters are kept whatever else the launch commits
__device__ __forceinline__ void smb_ready_count(SmbEnvState &S, int spent) {
  S.iters_total += spent;
  S.iters_max = max(S.iters_max, spent);
}

// A fresh episode on the map in L.map (stored already, its observation written): the counters, then the search with what the
// launch has left.  True when it finished (statistics and last_loss are set, as smb_env_begin sets them); false leaves the env
// with pending statistics.  Every lane holds the same S.
template <class CtrlLds>
__device__ inline bool smb_ready_begin(SmbLds &L, const SmbReadyArgs &ra, int env, SmbEnvState &S, const int *pos, int &left,
                                       CtrlLds &C) {
  const SmbEnvArgs &a = ra.e;
  SmbResult r;
  smb_scan_level(L, a.h, a.w, r);
  S.pos[0] = pos[0];
  S.pos[1] = pos[1];
  S.n_step = S.iteration = S.changes = S.ep_len = 0;
  S.ep_return = 0.0;
  // the queued or resampled targets are committed by the launch that brings the new level, whenever its search ends
  smb_ctrl_take(C, a.ctrl, env, threadIdx.x & 63);
  if (!smb_play_budgeted(L, a.h, a.w, a.power, smb_env_nodes(a, env), smb_env_heap(a, env), ra.park + env, false, left, r))
    return false;
#pragma unroll
  for (int k = 0; k < SMB_STATS; k++) S.stats[k] = r.stats[k];
  S.searches++;
  S.last_loss = smb_env_loss(a, S.stats, C);
  return true;
}

#ifndef PCGRL_SMB_READY_DEVICE_ONLY  // (smb/pcgrl_k_smb_state.hip takes the device functions above without a second set of kernels)
template <bool CTRL>
__global__ __launch_bounds__(64) void smb_ready_reset_kernel(const SmbReadyArgs ra) {
  __shared__ SmbLds L;
  __shared__ typename SmbCtrlLdsOf<CTRL>::type C;
  const SmbEnvArgs &a = ra.e;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= a.n) return;
  const bool active = !a.mask || a.mask[env] != 0;
  SmbEnvState *Q = a.st + env;
  smb_ctrl_load(C, a.ctrl, env, lane);
  SmbEnvState S;  // what smb_ready_begin reads and writes; the last finished episode stays where it is
  S.searches = Q->searches;
  S.iters_total = Q->iters_total;
  S.iters_max = Q->iters_max;
  int pos[2] = {Q->pos[0], Q->pos[1]};
  if (!active) {  // the env stays as it is, parked search included, and gets no iterations; its row is the committed observation
    smb_env_load_map(L, a, env, lane);
    __syncthreads();
    smb_env_write_obs(L, a, env, lane, pos[0], pos[1]);
    if constexpr (CTRL) smb_ctrl_write_obs(C, a.ctrl, env, lane, Q->stats);
    return;
  }
  smb_env_reset_map(L, a, env, lane, pos);
  __syncthreads();
  smb_env_write_obs(L, a, env, lane, pos[0], pos[1]);
  smb_env_store_map(L, a, env, lane);
  int left = ra.budget;
  const bool finished = smb_ready_begin(L, ra, env, S, pos, left, C);  // whatever was in flight is abandoned: a fresh search
  smb_ready_count(S, ra.budget - left);
  if constexpr (CTRL) {  // (pending statistics: the old level's value until the search is over)
    if (finished) smb_ctrl_write_obs(C, a.ctrl, env, lane, S.stats);
    else smb_ctrl_write_obs(C, a.ctrl, env, lane, Q->stats);
  }
  if (lane == 0) {
    ra.park[env].mode = finished ? SMB_READY_IDLE : SMB_READY_PENDING_STATS;
    smb_env_commit_reset(Q, S, finished);
  }
}

template <bool CTRL>
__global__ __launch_bounds__(64) void smb_ready_step_kernel(const SmbReadyArgs ra) {
  __shared__ SmbLds L;
  __shared__ typename SmbCtrlLdsOf<CTRL>::type C;
  const SmbEnvArgs &a = ra.e;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= a.n) return;
  const int H = a.h, W = a.w;
  smb_env_load_map(L, a, env, lane);
  SmbEnvState S = a.st[env];
  smb_ctrl_load(C, a.ctrl, env, lane);
  SmbPark *P = ra.park + env;
  const int mode = P->mode;
  int left = ra.budget;
  uint2 *nodes = smb_env_nodes(a, env);
  uint32_t *heap = smb_env_heap(a, env);
  __syncthreads();
  if (mode == SMB_READY_PENDING_STATS) {  // the level of an episode that began in an earlier launch: no action is taken
    smb_env_write_obs(L, a, env, lane, S.pos[0], S.pos[1]);
    SmbResult r;
    smb_scan_level(L, H, W, r);
    const bool finished = smb_play_budgeted(L, H, W, a.power, nodes, heap, P, true, left, r);
    smb_ready_count(S, ra.budget - left);
    if (finished) {
#pragma unroll
      for (int k = 0; k < SMB_STATS; k++) S.stats[k] = r.stats[k];
      S.searches++;
      S.last_loss = smb_env_loss(a, S.stats, C);  // the targets the launch that brought the level committed
    }
    smb_ctrl_write_obs(C, a.ctrl, env, lane, S.stats);
    if (lane == 0) {
      if (finished) P->mode = SMB_READY_IDLE;
      a.st[env] = S;
      ra.status[env] = finished ? (uint8_t)0 : (uint8_t)PCGRL_ENV_BUSY;
    }
    return;
  }
  const bool resume = mode == SMB_READY_PENDING_STEP;
  const int act = resume ? P->action : a.actions[env];
  // (an idle env only: a parked action was checked when it was taken)
  if (smb_env_bad_action(a, act, a.rep == PCGRL_REP_NARROW ? SMB_TILES : 4 + SMB_TILES, env, lane, S)) {
    if (lane == 0) ra.status[env] = (uint8_t)PCGRL_ENV_EMITTED;
    smb_env_write_obs(L, a, env, lane, S.pos[0], S.pos[1]);
    smb_ctrl_write_obs(C, a.ctrl, env, lane, S.stats);
    return;
  }
  // the representation's update, on the LDS copy alone: the step is committed only when its search is over
  const int64_t iters_total = S.iters_total;
  const int iters_max = S.iters_max;
  SmbEnvEdit e = smb_env_update(L, a, act, lane, S);
  const bool renew = e.done && a.auto_reset != 0;
  // the observation of the step in flight, before the search: a busy env's row holds it (a renewing step writes it again below)
  if (!renew || e.resolid) smb_env_write_obs(L, a, env, lane, e.pos[0], e.pos[1]);
  if (e.changed) {  // smb_env_restat's two shortcuts, the search under the budget
    SmbResult r;
    smb_scan_level(L, H, W, r);
#pragma unroll
    for (int k = 0; k < 5; k++) S.stats[k] = r.stats[k];
    if (e.resolid) {
      if (!smb_play_budgeted(L, H, W, a.power, nodes, heap, P, resume, left, r)) {  // parked: nothing of the step is committed
        if (lane == 0) {
          if (!resume) {
            P->mode = SMB_READY_PENDING_STEP;
            P->action = act;
          }
          a.st[env].iters_total = iters_total + ra.budget;  // a parked launch spent all it had
          a.st[env].iters_max = max(iters_max, ra.budget);
          ra.status[env] = (uint8_t)PCGRL_ENV_BUSY;
        }
        return;
      }
#pragma unroll
      for (int k = 5; k < SMB_STATS; k++) S.stats[k] = r.stats[k];
      S.searches++;
    }
    smb_env_store_map(L, a, env, lane);  // only now: nothing of a parked step is committed
  }
  smb_env_emit(a, env, lane, e, S, C);
  if (e.done) smb_env_latch(S);
  int next_mode = SMB_READY_IDLE;
  if (renew) {  // the next episode inside the same launch, its search with what the launch has left
    __syncthreads();
    smb_env_draw(L, a, env, lane, e.pos);
    __syncthreads();
    smb_env_write_obs(L, a, env, lane, e.pos[0], e.pos[1]);
    smb_env_store_map(L, a, env, lane);
    if (!smb_ready_begin(L, ra, env, S, e.pos, left, C)) next_mode = SMB_READY_PENDING_STATS;
  }
  smb_ready_count(S, ra.budget - left);
  smb_ctrl_write_obs(C, a.ctrl, env, lane, S.stats);
  if (lane == 0) {
    if (next_mode != mode) P->mode = next_mode;
    a.st[env] = S;
    ra.status[env] = (uint8_t)(PCGRL_ENV_EMITTED | (next_mode != SMB_READY_IDLE ? PCGRL_ENV_BUSY : 0));
  }
}

__global__ __launch_bounds__(256) void smb_ready_busy_kernel(const SmbPark *park, int n, uint8_t *busy) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env < n) busy[env] = park[env].mode != SMB_READY_IDLE ? 1 : 0;
}

#endif  // PCGRL_SMB_READY_DEVICE_ONLY

#endif  // PCGRL_KERNEL_TU

}  // namespace pcgrl
