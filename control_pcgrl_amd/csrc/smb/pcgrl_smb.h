// smb/pcgrl_smb.h -- Super Mario Bros levels on the device (include/pcgrl_amd_smb.h): what SMBCtrlProblem.get_stats
// computes for an H x W map of 7 tile types (envs/probs/smb/smb_prob.py:132-154) -- five map statistics and an A* play-through
// of the level (smb/engine.py) -- and the loss ControlWrapper.get_loss derives from them.  DESIGN.md section 17 has the rules
// with every quirk; tests/smb_rules.py is the same in plain Python.
//
// smb_kernel: one 64-lane wave per level.
//   map       the level's bytes are staged in LDS (ids above 6 become 0 and raise error bit 0); smb_evaluate_level takes that
//             LDS map, so the step kernel of smb/pcgrl_smb_env.h calls it (or its scan half alone) on the map it already holds.
//   scans     lane-parallel: a lane owns columns `lane` and `lane + 64` (W <= 128), walks each bottom-up once (nearest floor
//             below for dist-floor, both neighbour comparisons for noise, the tube's two side neighbours, the two counts) and
//             leaves the column's 16-bit solid mask in LDS; five wave reductions.
//   level     col[x], 0 <= x < W + 6: bit y = solid.  The three columns on each side hold rows H-2, H-1; col[W + 4] also H-3.
//   search    lane 0 alone.  What a search iteration costs is the chain of dependent loads of the heap's sifts, which the four
//             children in four lanes or a level per lane would not shorten (a level per lane would also keep 64 x 4.5 KB of
//             LDS per wave, one wave per CU); the latency is hidden by occupancy instead -- 4.5 KB of LDS and one wave per
//             level let a CU hold 32 levels.  The open list is CPython's heapq (heappush = append + _siftdown, heappop =
//             move the last item to the root, _siftup to a leaf along the smaller children, _siftdown back), ordered by f
//             alone with `<`, because the sift order decides which of several equal-f nodes is expanded first: pt_heap_push<17>
//             and pt_heap_pop<17> of playthrough/pcgrl_playthrough.h, which the Dave and MiniDungeon solvers use at 16 bits.  The loop body is
//             smb_search_iteration, the start smb_search_start and the finished search's tail smb_play_result: the budgeted,
//             resumable search of smb/pcgrl_smb_ready.h runs the same three.
//   memory    per level a workspace slot in HBM: nodes (8 B: x 8 | y+5 5 | airTime 3 | jumps 14 | action 2 ; parent 17 |
//             depth 14) and heap entries (4 B: f 15 | node 17), 4 * power + 1 of each -- an expansion pushes four, and there
//             are at most `power` expansions.  Both arrays are written before they are read (count-bounded), so a dirty
//             workspace does not matter.  The visited set is an LDS bit set over (x, y + 5, airTime): 134 * 21 * 6 bits.
//   outputs   the final node's parent chain gives the moves, the jump locations (a node jumped iff its count exceeds its
//             parent's; the location is the parent's position) and jumps-dist (walked backwards: W - x_J, x_J - x_{J-1}, ...,
//             x_1 - 0); all lanes fill the tails with -1.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../playthrough/pcgrl_playthrough.h"  // pt_heap_push, pt_heap_pop, pt_wave_sum

namespace pcgrl {

constexpr int SMB_TILES = 7;
constexpr int SMB_STATS = 9;  // dist-floor, disjoint-tubes, enemies, empty, noise, jumps, jumps-dist, dist-win, sol-length
constexpr int SMB_MAX_H = 16, SMB_MIN_H = 4, SMB_MAX_W = 128;
constexpr int SMB_MAX_POWER = 16000;  // depth, jumps < 2^14; f < 2^15; 4 * power + 1 nodes < 2^17
constexpr int SMB_MAX_LW = SMB_MAX_W + 6;
constexpr int SMB_SEEN_WORDS = (SMB_MAX_LW * 21 * 6 + 31) / 32;  // 528
constexpr uint32_t SMB_NO_PARENT = 0x1FFFFu;

struct SmbArgs {
  int32_t h, w, power, n;
  const uint8_t *grids;  // uint8 [n][h][w]
  uint8_t *ws;           // n slots of ws_stride bytes
  int64_t ws_stride;
  int32_t cap, jump_cap;
  int32_t *stats;        // [n][9]
  double *loss;          // [n] or null
  int8_t *moves;         // [n][cap] or null
  int32_t *length;       // [n] or null
  int16_t *jump_locs;    // [n][jump_cap][2] or null
  int32_t *play;         // [n][6] or null
  uint32_t *error;       // [n] or null
  int32_t has_trg[SMB_STATS];
  double weight[SMB_STATS], trg_lo[SMB_STATS], trg_hi[SMB_STATS];
};

__host__ __device__ inline int64_t smb_nodes_per_pass(int power) { return 4 * (int64_t)power + 1; }
// one level's workspace slot: the nodes, then the heap; a multiple of 16 bytes
inline int64_t smb_ws_stride(int power) { return (smb_nodes_per_pass(power) * 12 + 15) / 16 * 16; }

hipError_t launch_smb(const SmbArgs &a, hipStream_t s);

#ifdef PCGRL_KERNEL_TU

struct SmbLds {
  uint8_t map[SMB_MAX_H * SMB_MAX_W];
  uint16_t col[SMB_MAX_LW + 2];
  uint32_t seen[SMB_SEEN_WORDS];
};

// what one level's evaluation leaves (every lane holds the same values)
struct SmbResult {
  int32_t stats[SMB_STATS];
  int32_t won, x, y, air, it1, it2, length;
};

// where one level's play-through goes; any pointer may be null
struct SmbPlayOut {
  int8_t *moves;
  int16_t *jump_locs;
  int32_t cap, jump_cap;
};

// a map byte as the kernels read it: a tile id above 6 reads as empty and sets `bad` (the caller raises its error bit)
__device__ __forceinline__ uint8_t smb_tile(uint8_t t, bool &bad) {
  if (t >= SMB_TILES) {
    bad = true;
    return 0;
  }
  return t;
}

// One term of ControlWrapper.get_loss: -(distance of the statistic to its zero-loss interval [lo, hi]) * weight, rounded to
// double before it is added (no fused multiply-add): the Python rules bit for bit whatever the targets.
__device__ __forceinline__ double smb_target_term(int32_t stat, double lo, double hi, double weight) {
#pragma clang fp contract(off)
  const double v = (double)stat;
  const double d = v < lo ? lo - v : (v > hi ? v - hi : 0.0);
  return -d * weight;
}

// ControlWrapper.get_loss: the terms of the statistics that have a target, added in the statistics' order.  Unrolled, for the
// callers that hold the statistics in registers.
__device__ __forceinline__ double smb_target_loss(const int32_t *has_trg, const double *weight, const double *lo, const double *hi,
                                                  const int32_t *stats) {
  double loss = 0.0;
#pragma unroll
  for (int k = 0; k < SMB_STATS; k++)
    if (has_trg[k]) loss = loss + smb_target_term(stats[k], lo[k], hi[k], weight[k]);
  return loss;
}

__device__ __forceinline__ bool smb_movable(const uint16_t *col, int H, int LW, int x, int y) {
  if (y < 0) return true;  // checkMovableLocation: above the level everything is free, whatever x
  if (x >= LW || y >= H) return false;
  return ((col[x] >> y) & 1u) == 0;
}

__device__ __forceinline__ uint2 smb_pack(int x, int y, int air, int jumps, int action, uint32_t parent, int depth) {
  return make_uint2((uint32_t)x | ((uint32_t)(y + 5) << 8) | ((uint32_t)air << 13) | ((uint32_t)jumps << 16) |
                        ((uint32_t)action << 30),
                    parent | ((uint32_t)depth << 17));
}
__device__ __forceinline__ int smb_nx(uint2 v) { return v.x & 0xFF; }
__device__ __forceinline__ int smb_ny(uint2 v) { return (int)((v.x >> 8) & 0x1F) - 5; }
__device__ __forceinline__ int smb_nair(uint2 v) { return (v.x >> 13) & 7; }
__device__ __forceinline__ int smb_njumps(uint2 v) { return (v.x >> 16) & 0x3FFF; }
__device__ __forceinline__ int smb_naction(uint2 v) { return v.x >> 30; }
__device__ __forceinline__ uint32_t smb_nparent(uint2 v) { return v.y & 0x1FFFFu; }
__device__ __forceinline__ int smb_ndepth(uint2 v) { return v.y >> 17; }

// A search before its first iteration: the start node alone in the open list, nothing expanded and no best node yet.  The
// caller's lanes take the loop's words; nodes[0] and heap[0] are written by the lane(s) that call it with `write`.  This is also
// what "parked after 0 iterations" means (smb/pcgrl_smb_ready.h, smb/pcgrl_smb_state.h), with a zeroed visited set.
__device__ __forceinline__ void smb_search_start(uint2 *nodes, uint32_t *heap, int H, int W, bool write, int &it, int &nn, int &hn,
                                                 uint32_t &best, int &best_x, int &best_depth) {
  if (write) {
    nodes[0] = smb_pack(1, H - 3, 0, 0, 0, SMB_NO_PARENT, 0);
    heap[0] = (uint32_t)(W + 4 - 1) << 17;
  }
  it = 0, nn = 1, hn = 1, best = 0, best_x = -1, best_depth = 0;
}

// One iteration of AStarAgent.getSolution's loop (one lane): pops the open list's first node and expands it; true when that node
// wins (`best` is then the winner).  The only A* loop body of the library: smb_search runs it to the end, smb_play_budgeted of
// smb/pcgrl_smb_ready.h under a launch's budget.
__device__ __forceinline__ bool smb_search_iteration(const uint16_t *col, uint32_t *seen, uint2 *nodes, uint32_t *heap, int H,
                                                     int LW, int ex, int balance, int &nn, int &hn, uint32_t &best, int &best_x,
                                                     int &best_depth) {
  const uint32_t cur = pt_heap_pop<17>(heap, hn) & 0x1FFFFu;
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
    pt_heap_push<17>(heap, hn, ((uint32_t)((ex - cx) + balance * (depth + 1)) << 17) | (uint32_t)nn);
    nn++;
  }
  return false;
}

// AStarAgent.getSolution on the level in col[] (one lane): returns the node it ends on -- the winner, else the best node --
// and the iterations it ran.  `seen` must be zero on entry.
__device__ inline uint32_t smb_search(const uint16_t *col, uint32_t *seen, uint2 *nodes, uint32_t *heap, int H, int W, int power,
                                      int balance, int &iterations, bool &won) {
  int it, nn, hn, best_x, best_depth;
  uint32_t best;
  smb_search_start(nodes, heap, H, W, true, it, nn, hn, best, best_x, best_depth);
  won = false;
  while (it < power && hn > 0) {
    it++;
    if (smb_search_iteration(col, seen, nodes, heap, H, W + 6, W + 4, balance, nn, hn, best, best_x, best_depth)) {
      won = true;
      break;
    }
  }
  iterations = it;
  return best;
}

// The scan half of a level's evaluation, by one 64-lane wave: the five map statistics of the map in L.map ([H][W], ids 0..6)
// into r.stats[0..4], and the level's solid columns into L.col.  The step kernel of smb/pcgrl_smb_env.h calls it alone when an
// edit left the level's solidity as it was (the play statistics keep their values then).
__device__ inline void smb_scan_level(SmbLds &L, int H, int W, SmbResult &r) {
  const int lane = threadIdx.x & 63;
  int dist_floor = 0, tubes = 0, enemies = 0, empty = 0, noise = 0;
  for (int x = lane; x < W; x += 64) {
    int floor_y = -1;  // the nearest floor tile below the current row
    uint32_t mask = 0;
    int below = -1;
    for (int y = H - 1; y >= 0; y--) {
      const int t = L.map[y * W + x];
      if (t == 2) {
        enemies++;
        dist_floor += floor_y >= 0 ? floor_y - y - 1 : H - 1;
      }
      empty += t == 0;
      if (t == 6) {
        const int nb = (x > 0 && L.map[y * W + x - 1] == 6) + (x < W - 1 && L.map[y * W + x + 1] == 6);
        tubes += nb == 1;
      }
      if (x > 0) noise += t != L.map[y * W + x - 1];
      if (below >= 0) noise += t != below;
      below = t;
      if (t == 1 || t == 3 || t == 4) floor_y = y;  // tubes are not floor
      if (t == 1 || t == 3 || t == 4 || t == 6) mask |= 1u << y;
    }
    L.col[x + 3] = (uint16_t)mask;
  }
  if (lane < 6) {
    const uint32_t border = 3u << (H - 2);
    const int x = lane < 3 ? lane : W + lane;
    L.col[x] = (uint16_t)(border | (x == W + 4 ? 1u << (H - 3) : 0u));
  }
  r.stats[0] = pt_wave_sum(dist_floor);
  r.stats[1] = pt_wave_sum(tubes);
  r.stats[2] = pt_wave_sum(enemies);
  r.stats[3] = pt_wave_sum(empty);
  r.stats[4] = pt_wave_sum(noise);
}

// What a finished play-through leaves: the chain of its final node `fin` gives r.stats[5..8] (jumps, jumps-dist, dist-win,
// sol-length) and the play record in `out` (empty: nothing is written).  fin, it1 and it2 are lane 0's values, `won` every
// lane's.  Every lane returns with the same values.
__device__ __forceinline__ void smb_play_result(int W, const uint2 *nodes, uint32_t fin, int won, int it1, int it2,
                                                const SmbPlayOut &out, SmbResult &r) {
  const int lane = threadIdx.x & 63;
  // the final node's chain, by lane 0
  int fx = 0, fy = 0, fair = 0, fj = 0, fdepth = 0, jdist = 0;
  if (lane == 0) {
    uint2 nd = nodes[fin];
    fx = smb_nx(nd), fy = smb_ny(nd), fair = smb_nair(nd), fj = smb_njumps(nd), fdepth = smb_ndepth(nd);
    int next_x = W;
    for (int p = fdepth - 1; p >= 0; p--) {
      const uint2 par = nodes[smb_nparent(nd)];
      if (out.moves && p < out.cap) out.moves[p] = (int8_t)smb_naction(nd);
      const int j = smb_njumps(nd);
      if (j > smb_njumps(par)) {  // this move jumped, from the parent's position
        const int jx = smb_nx(par);
        if (out.jump_locs && j - 1 < out.jump_cap) {
          out.jump_locs[2 * (j - 1)] = (int16_t)jx;
          out.jump_locs[2 * (j - 1) + 1] = (int16_t)smb_ny(par);
        }
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
  r.it1 = __shfl(it1, 0, 64);
  r.it2 = __shfl(it2, 0, 64);
  r.length = __shfl(fdepth, 0, 64);
  r.stats[5] = __shfl(fj, 0, 64);
  r.stats[6] = __shfl(jdist, 0, 64);
  r.stats[7] = won ? 0 : (W + 4) - r.x;
  r.stats[8] = won ? r.length : 0;
  if (out.moves)
    for (int p = max(r.length, 0) + lane; p < out.cap; p += 64) out.moves[p] = -1;
  if (out.jump_locs)
    for (int j = r.stats[5] + lane; j < out.jump_cap; j += 64) {
      out.jump_locs[2 * j] = -1;
      out.jump_locs[2 * j + 1] = -1;
    }
}

// The play half: the A* play-through of the level in L.col (smb_scan_level left it there) into r.stats[5..8] and the play record.
// nodes / heap: this level's workspace slot.  Every lane returns with the same values.
__device__ inline void smb_play_level(SmbLds &L, int H, int W, int power, uint2 *nodes, uint32_t *heap, const SmbPlayOut &out,
                                      SmbResult &r) {
  const int lane = threadIdx.x & 63;
  uint32_t fin = 0;
  int it1 = 0, it2 = 0, won = 0;
  for (int pass = 0; pass < 2; pass++) {
    for (int i = lane; i < SMB_SEEN_WORDS; i += 64) L.seen[i] = 0;
    __syncthreads();
    if (lane == 0) {
      bool w;
      int it;
      fin = smb_search(L.col, L.seen, nodes, heap, H, W, power, pass == 0 ? 1 : 0, it, w);
      won = w ? 1 : 0;
      if (pass == 0) it1 = it;
      else it2 = it;
    }
    won = __shfl(won, 0, 64);
    __syncthreads();
    if (won) break;
  }
  smb_play_result(W, nodes, fin, won, it1, it2, out, r);
}

// One level, by one 64-lane wave: the nine statistics and the play-through of the map in L.map ([H][W], ids 0..6).
// nodes / heap: this level's workspace slot.  Every lane returns with the same SmbResult.
__device__ inline void smb_evaluate_level(SmbLds &L, int H, int W, int power, uint2 *nodes, uint32_t *heap, const SmbPlayOut &out,
                                          SmbResult &r) {
  smb_scan_level(L, H, W, r);
  smb_play_level(L, H, W, power, nodes, heap, out, r);
}

#ifndef PCGRL_SMB_DEVICE_ONLY  // (smb/pcgrl_k_smb_env.hip takes the device functions above without a second smb_kernel)
__global__ __launch_bounds__(64) void smb_kernel(const SmbArgs a) {
  __shared__ SmbLds L;
  const int lvl = blockIdx.x, lane = threadIdx.x;
  if (lvl >= a.n) return;
  const int H = a.h, W = a.w, cells = H * W;
  const uint8_t *g = a.grids + (size_t)lvl * cells;
  bool bad = false;
  for (int i = lane; i < cells; i += 64) L.map[i] = smb_tile(g[i], bad);
  const uint32_t err = __any(bad) ? 1u : 0u;
  __syncthreads();
  uint8_t *slot = a.ws + (size_t)lvl * a.ws_stride;
  uint2 *nodes = (uint2 *)slot;
  uint32_t *heap = (uint32_t *)(slot + smb_nodes_per_pass(a.power) * 8);
  SmbPlayOut out;
  out.moves = a.moves ? a.moves + (size_t)lvl * a.cap : nullptr;
  out.jump_locs = a.jump_locs ? a.jump_locs + (size_t)lvl * a.jump_cap * 2 : nullptr;
  out.cap = a.cap;
  out.jump_cap = a.jump_cap;
  SmbResult r;
  smb_evaluate_level(L, H, W, a.power, nodes, heap, out, r);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < SMB_STATS; k++) a.stats[(size_t)lvl * SMB_STATS + k] = r.stats[k];
    if (a.loss) {
      // smb_target_loss as a loop: unrolled, the targets' 63 argument words are live at once, and at 106 scalar registers
      // instead of 76 a SIMD holds six of this kernel's waves, not eight
      double loss = 0.0;
      for (int k = 0; k < SMB_STATS; k++)
        if (a.has_trg[k]) loss = loss + smb_target_term(r.stats[k], a.trg_lo[k], a.trg_hi[k], a.weight[k]);
      a.loss[lvl] = loss;
    }
    if (a.length) a.length[lvl] = r.length;
    if (a.play) {
      int32_t *p = a.play + (size_t)lvl * 6;
      p[0] = r.won, p[1] = r.x, p[2] = r.y, p[3] = r.air, p[4] = r.it1, p[5] = r.it2;
    }
    if (a.error) a.error[lvl] = err;
  }
}
#endif  // PCGRL_SMB_DEVICE_ONLY

#endif  // PCGRL_KERNEL_TU

}  // namespace pcgrl
