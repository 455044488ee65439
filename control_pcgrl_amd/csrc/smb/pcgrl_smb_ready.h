// smb/pcgrl_smb_ready.h -- asynchronous stepping of Super Mario Bros environments (include/pcgrl_amd_smb_ready.h): the step and
// reset kernels of smb/pcgrl_smb_env.h with a budgeted, resumable A* play-through.  DESIGN.md section 19 has the launch rules;
// tests/smb_ready_rules.py is the same in plain Python.
//
// One 64-lane wave per env, as the synchronous kernels; a launch gives every env `budget` search iterations.
//   search    smb_play_budgeted runs smb_ready_iteration -- the loop body of smb_search of smb/pcgrl_smb.h, same pops, same
//             pushes, same visited set -- on lane 0 until the search is over (won, it == power, open list empty) or the launch's iterations are spent.
//             Pass 2 starts in the same launch with what is left.  A search whose last iteration spends the budget is over.
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
//             iterations", the start of a search of the map it has just stored.  The envs outside their masks keep both.
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

// One iteration of AStarAgent.getSolution's loop (one lane): pops the open list's first node and expands it; true when that node
// wins (`best` is then the winner).  This is the body of smb_search's loop in smb/pcgrl_smb.h, statement for statement, with
// `continue` written as `return false`: the synchronous kernels keep their own copy so that their compiled form stays what it
// was, and the test that steps both side by side under a budget no search exceeds holds the two together.
__device__ __forceinline__ bool smb_ready_iteration(const uint16_t *col, uint32_t *seen, uint2 *nodes, uint32_t *heap, int H,
                                                     int LW, int ex, int balance, int &nn, int &hn, uint32_t &best, int &best_x,
                                                     int &best_depth) {
  const uint32_t cur = smb_heap_pop(heap, hn) & 0x1FFFFu;
  const uint2 nd = nodes[cur];
  const int x = smb_nx(nd), y = smb_ny(nd), air = smb_nair(nd), jumps = smb_njumps(nd), depth = smb_ndepth(nd);
  if (y >= H) return false;  // a lose node
  if (x >= ex) {
    best = cur;
    return true;
  }
  const int bit = (x * 21 + (y + 5)) * 6 + air;
  if ((seen[bit >> 5] >> (bit & 31)) & 1u) return false;
  if (x > best_x || (x == best_x && depth < best_depth)) {  // a smaller ex - x, or the same with a smaller depth
    best = cur;
    best_x = x;
    best_depth = depth;
  }
  seen[bit >> 5] |= 1u << (bit & 31);
  // State.update for the four actions (dx, dy) = (0,0), (1,0), (0,-1), (1,-1)
  const bool ground = (y >= -1 && y < H - 1) ? ((col[x] >> (y + 1)) & 1u) != 0 : false;
  const bool right = smb_movable(col, H, LW, x + 1, y);
  for (int a = 0; a < 4; a++) {
    const int cx = ((a & 1) && right) ? x + 1 : x;
    int cy = y, cair = air, cj = jumps;
    if (a & 2) {
      if (ground && smb_movable(col, H, LW, cx, y - 1)) {
        cair = 5;
        cj++;
      }
    } else if (cair > 0) {
      cair = 1;
    }
    if (cair > 1) {
      cair--;
      if (smb_movable(col, H, LW, cx, y - 1)) cy = y - 1;
      else cair = 1;
    } else if (cair == 1) {
      cair = 0;
    } else if (smb_movable(col, H, LW, cx, y + 1)) {
      cy = y + 1;
    }
    nodes[nn] = smb_pack(cx, cy, cair, cj, a, cur, depth + 1);
    smb_heap_push(heap, hn, ((uint32_t)((ex - cx) + balance * (depth + 1)) << 17) | (uint32_t)nn);
    nn++;
  }
  return false;
}

// What a finished play-through leaves, as the tail of smb_play_level without a play record: the chain of its final node `fin`
// (lane 0's value) into r.stats[5..8].  Every lane returns with the same values.
__device__ __forceinline__ void smb_ready_result(int W, const uint2 *nodes, uint32_t fin, int won, int it1, int it2, SmbResult &r) {
  const int lane = threadIdx.x & 63;
  int fx = 0, fy = 0, fair = 0, fj = 0, fdepth = 0, jdist = 0;
  if (lane == 0) {
    uint2 nd = nodes[fin];
    fx = smb_nx(nd), fy = smb_ny(nd), fair = smb_nair(nd), fj = smb_njumps(nd), fdepth = smb_ndepth(nd);
    int next_x = W;
    for (int p = fdepth - 1; p >= 0; p--) {
      const uint2 par = nodes[smb_nparent(nd)];
      if (smb_njumps(nd) > smb_njumps(par)) {  // this move jumped, from the parent's position
        const int jx = smb_nx(par);
        jdist = max(jdist, next_x - jx);
        next_x = jx;
      }
      nd = par;
    }
    jdist = max(jdist, next_x);
  }
  r.won = won;
  r.x = __shfl(fx, 0, 64);
  r.y = __shfl(fy, 0, 64);
  r.air = __shfl(fair, 0, 64);
  r.it1 = it1;
  r.it2 = it2;
  r.length = __shfl(fdepth, 0, 64);
  r.stats[5] = __shfl(fj, 0, 64);
  r.stats[6] = __shfl(jdist, 0, 64);
  r.stats[7] = won ? 0 : (W + 4) - r.x;
  r.stats[8] = won ? r.length : 0;
}

// The play half of a level's evaluation under a budget: `left` iterations may still run in this launch (it comes back with what
// the search left over).  resume: continue the search parked in P, else start one.  True when the search is over: r.stats[5..8]
// and the play record are then set as smb_play_level sets them.  False: the search is parked in P (the loop's words and the
// visited set; the caller sets mode and action).  Every lane returns with the same values.
__device__ inline bool smb_play_budgeted(SmbLds &L, int H, int W, int power, uint2 *nodes, uint32_t *heap, SmbPark *P, bool resume,
                                         int &left, SmbResult &r) {
  const int lane = threadIdx.x & 63;
  const int LW = W + 6, ex = W + 4;
  int pass = 0, it = 0, nn = 1, hn = 1, best_x = -1, best_depth = 0, it1 = 0;
  uint32_t best = 0;
  if (resume) {
    pass = P->pass, it = P->it, nn = P->nn, hn = P->hn, best = P->best, best_x = P->best_x, best_depth = P->best_depth;
    it1 = P->it1;
    for (int i = lane; i < SMB_SEEN_WORDS; i += 64) L.seen[i] = P->seen[i];
  } else {
    for (int i = lane; i < SMB_SEEN_WORDS; i += 64) L.seen[i] = 0;
    if (lane == 0) {
      nodes[0] = smb_pack(1, H - 3, 0, 0, 0, SMB_NO_PARENT, 0);
      heap[0] = (uint32_t)(ex - 1) << 17;
    }
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
        if (smb_ready_iteration(L.col, L.seen, nodes, heap, H, LW, ex, balance, nn, hn, best, best_x, best_depth)) {
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
    pass = 1, it = 0, nn = 1, hn = 1, best = 0, best_x = -1, best_depth = 0;
    for (int i = lane; i < SMB_SEEN_WORDS; i += 64) L.seen[i] = 0;
    if (lane == 0) {
      nodes[0] = smb_pack(1, H - 3, 0, 0, 0, SMB_NO_PARENT, 0);
      heap[0] = (uint32_t)(ex - 1) << 17;
    }
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
  smb_ready_result(W, nodes, best, won, pass == 0 ? it : it1, pass == 0 ? 0 : it, r);
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
  uint8_t *slot = a.ws + (size_t)env * a.ws_stride;
  SmbResult r;
  smb_scan_level(L, a.h, a.w, r);
  S.pos[0] = pos[0];
  S.pos[1] = pos[1];
  S.n_step = S.iteration = S.changes = S.ep_len = 0;
  S.ep_return = 0.0;
  // the queued or resampled targets are committed by the launch that brings the new level, whenever its search ends
  smb_ctrl_take(C, a.ctrl, env, threadIdx.x & 63);
  if (!smb_play_budgeted(L, a.h, a.w, a.power, (uint2 *)slot, (uint32_t *)(slot + smb_nodes_per_pass(a.power) * 8), ra.park + env,
                         false, left, r))
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
  const int H = a.h, W = a.w, cells = H * W;
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
  for (int i = cells + lane; i < a.map_stride; i += 64) L.map[i] = 0;  // the padding of the stored row
  if (a.init_grids) {
    const uint8_t *g = a.init_grids + (size_t)env * cells;
    bool bad = false;
    for (int i = lane; i < cells; i += 64) {
      uint8_t t = g[i];
      if (t >= SMB_TILES) {
        t = 0;
        bad = true;
      }
      L.map[i] = t;
    }
    if (__any(bad) && lane == 0) atomicOr(a.err, 2);
    pos[0] = pos[1] = 0;
    if (a.init_pos && a.rep == PCGRL_REP_TURTLE) {
      pos[0] = min(max(a.init_pos[(size_t)env * 2], 0), H - 1);
      pos[1] = min(max(a.init_pos[(size_t)env * 2 + 1], 0), W - 1);
    }
  } else {
    smb_env_draw(L, a, env, lane, pos);
  }
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
    Q->pos[0] = S.pos[0];
    Q->pos[1] = S.pos[1];
    Q->n_step = Q->iteration = Q->changes = Q->ep_len = 0;
    Q->iters_total = S.iters_total;
    Q->iters_max = S.iters_max;
    Q->ep_return = 0.0;
    if (finished) {  // pending statistics keep the old ones until the search is over
      Q->searches = S.searches;
      Q->last_loss = S.last_loss;
#pragma unroll
      for (int k = 0; k < SMB_STATS; k++) Q->stats[k] = S.stats[k];
    }
  }
}

template <bool CTRL>
__global__ __launch_bounds__(64) void smb_ready_step_kernel(const SmbReadyArgs ra) {
  __shared__ SmbLds L;
  __shared__ typename SmbCtrlLdsOf<CTRL>::type C;
  const SmbEnvArgs &a = ra.e;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= a.n) return;
  const int H = a.h, W = a.w, cells = H * W;
  smb_env_load_map(L, a, env, lane);
  SmbEnvState S = a.st[env];
  smb_ctrl_load(C, a.ctrl, env, lane);
  SmbPark *P = ra.park + env;
  const int mode = P->mode;
  int left = ra.budget;
  uint8_t *slot = a.ws + (size_t)env * a.ws_stride;
  uint2 *nodes = (uint2 *)slot;
  uint32_t *heap = (uint32_t *)(slot + smb_nodes_per_pass(a.power) * 8);
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
  const int n_act = a.rep == PCGRL_REP_NARROW ? SMB_TILES : 4 + SMB_TILES;
  if (act < 0 || act >= n_act) {  // pcgrl_smb_env_step's rule: the error bit, and the env as it was (an idle env only)
    if (lane == 0) {
      atomicOr(a.err, 1);
      if (a.reward) a.reward[env] = 0.0f;
      if (a.reward64) a.reward64[env] = 0.0;
      if (a.done) a.done[env] = 0;
      if (a.stats_out)
        for (int k = 0; k < SMB_STATS; k++) a.stats_out[(size_t)env * SMB_STATS + k] = S.stats[k];
      ra.status[env] = (uint8_t)PCGRL_ENV_EMITTED;
    }
    smb_env_write_obs(L, a, env, lane, S.pos[0], S.pos[1]);
    smb_ctrl_write_obs(C, a.ctrl, env, lane, S.stats);
    return;
  }
  // the representation's update, on the LDS copy alone: the step is committed only when its search is over
  const int64_t iters_total = S.iters_total;
  const int iters_max = S.iters_max;
  int pos[2] = {S.pos[0], S.pos[1]};
  int tile = -1;
  if (a.rep == PCGRL_REP_NARROW) {
    tile = act;
  } else if (act < 4) {
    const int dr = act == 0 ? -1 : (act == 1 ? 1 : 0), dc = act == 2 ? -1 : (act == 3 ? 1 : 0);
    pos[0] = min(max(pos[0] + dr, 0), H - 1);
    pos[1] = min(max(pos[1] + dc, 0), W - 1);
  } else {
    tile = act - 4;
  }
  bool changed = false, resolid = false;
  if (tile >= 0) {
    const int idx = pos[0] * W + pos[1];
    const int old = L.map[idx];
    changed = old != tile;
    resolid = smb_tile_solid(old) != smb_tile_solid(tile);
    __syncthreads();
    if (lane == 0) L.map[idx] = (uint8_t)tile;
    __syncthreads();
  }
  if (a.rep == PCGRL_REP_NARROW) {
    const int c = S.n_step % cells;
    pos[0] = c / W;
    pos[1] = c % W;
    S.n_step++;
  }
  S.iteration++;
  S.changes += changed ? 1 : 0;
  S.ep_len++;
  bool done = S.iteration > a.max_iterations;
  if (a.max_changes >= 0) done = done || S.changes > a.max_changes;
  const bool renew = done && a.auto_reset != 0;
  // the observation of the step in flight, before the search: a busy env's row holds it (a renewing step writes it again below)
  if (!renew || resolid) smb_env_write_obs(L, a, env, lane, pos[0], pos[1]);
  if (changed) {
    SmbResult r;
    smb_scan_level(L, H, W, r);
#pragma unroll
    for (int k = 0; k < 5; k++) S.stats[k] = r.stats[k];
    if (resolid) {
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
    smb_env_store_map(L, a, env, lane);
  }
  const double loss = smb_env_loss(a, S.stats, C);
  const double reward = loss - S.last_loss;
  S.last_loss = loss;
  S.ep_return += reward;
  S.pos[0] = pos[0];
  S.pos[1] = pos[1];
  if (lane == 0) {
    if (a.reward) a.reward[env] = (float)reward;
    if (a.reward64) a.reward64[env] = reward;
    if (a.done) a.done[env] = done ? 1 : 0;
    if (a.stats_out)
      for (int k = 0; k < SMB_STATS; k++) a.stats_out[(size_t)env * SMB_STATS + k] = S.stats[k];
  }
  if (done) {
    S.last_return = S.ep_return;
    S.last_len = S.ep_len;
    S.last_count++;
#pragma unroll
    for (int k = 0; k < SMB_STATS; k++) S.last_stats[k] = S.stats[k];
  }
  int next_mode = SMB_READY_IDLE;
  if (renew) {  // the next episode inside the same launch, its search with what the launch has left
    __syncthreads();
    smb_env_draw(L, a, env, lane, pos);
    __syncthreads();
    smb_env_write_obs(L, a, env, lane, pos[0], pos[1]);
    smb_env_store_map(L, a, env, lane);
    if (!smb_ready_begin(L, ra, env, S, pos, left, C)) next_mode = SMB_READY_PENDING_STATS;
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
