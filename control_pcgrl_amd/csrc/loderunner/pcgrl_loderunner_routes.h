// loderunner/pcgrl_loderunner_routes.h -- the routes behind a Lode Runner level's path-length
// (include/pcgrl_amd_loderunner_routes.h): for every gold collected by its own pair of searches the cells of the two A* paths
// the reference's find_all_golds reads with Node.get_path (loderunner/engine.py:281-308) -- landing cell to gold, gold back to
// the landing cell -- laid end to end in gold order as the level's tour.  DESIGN.md section 28.
//
// loderunner_routes_kernel: loderunner_kernel's geometry, workspace and rules (one 64-lane wave per level, one search per
// lane; pcgrl_loderunner.h, whose device functions it composes: there is one lr_search and one accumulation loop) with a hook
// in lr_evaluate_level:
//   chain     a search leaves its parent chain in the lane's `cells` words; the goal is never closed, so lr_search hands its
//             parent out.  The chain stands until the lane's next search: the next round, or the next level of the block.
//   offsets   whether a pair counts is known only in the round's sequential accumulation.  That loop is uniform over the wave,
//             so at every pair that counts each lane sees the running length of the tour: the two lanes of the pair keep it as
//             their routes' offsets (the return route behind the outward one), lane 0 stores the gold's offset and return length.
//   emission  after the round's accumulation each lane with an offset walks its chain from the goal backwards and stores cell k
//             at offset + k: no reversal pass.  A move is a function of two neighbouring cells (the six moves have six different
//             steps), so it is derived from the cells, not stored by the search.
//   the rest  the wave fills [tour_len, route_cap) with -1, and the offsets of the golds without a route.
// Nothing is stored past route_cap or gold_cap; tour_len, the offsets below gold_cap and the statistics stay complete.
#pragma once
#include "pcgrl_loderunner.h"

namespace pcgrl {

struct LrRouteArgs {
  LrArgs lr;           // what loderunner_kernel takes
  int32_t route_cap;
  int16_t *coords;     // [n][route_cap][2] or null
  int8_t *moves;       // [n][route_cap] or null
  int32_t *tour_len;   // [n] or null
  int32_t *gold_off;   // [n][gold_cap] or null
  int16_t *gold_back;  // [n][gold_cap] or null
};

hipError_t launch_loderunner_routes(const LrRouteArgs &a, hipStream_t s);

#ifdef PCGRL_KERNEL_TU

// the move that leads from cell `from` to the neighbouring cell `to`: 0..5 = left right up down d-left d-right (lr_search's steps)
__device__ __forceinline__ int lr_move_between(int from, int to, int W) {
  const int dr = to / W - from / W, dc = to % W - from % W;
  if (dr == 0) return dc < 0 ? 0 : 1;
  if (dr < 0) return 2;
  return dc == 0 ? 3 : (dc < 0 ? 4 : 5);
}

// What loderunner_kernel stores for level `lvl` -- the per-gold record, the statistics, the loss, the play record and the error
// word -- in its words: that kernel keeps its text, so that its machine code stays what it was.  By all 64 lanes, after a
// barrier behind lr_evaluate_level.
__device__ __forceinline__ void lr_store_level(const LrArgs &a, const LrLds &L, const LrResult &r, int lvl, uint32_t err) {
  const int lane = threadIdx.x;
  if (a.gold_state)
    for (int j = lane; j < a.gold_cap; j += 64)
      a.gold_state[(size_t)lvl * a.gold_cap + j] = j < r.gold ? (int8_t)L.state[L.golds[j]] : (int8_t)-1;
  if (a.gold_dist)
    for (int j = lane; j < a.gold_cap; j += 64)
      a.gold_dist[(size_t)lvl * a.gold_cap + j] = j < r.gold ? (int16_t)L.dist[L.golds[j]] : (int16_t)0;
  if (lane == 0) {
    const double st[LR_STATS] = {(double)r.player, (double)r.enemies, (double)r.gold, r.win, (double)r.path_length};
    for (int k = 0; k < LR_STATS; k++) a.stats[(size_t)lvl * LR_STATS + k] = st[k];
    if (a.loss) {
      double loss = 0.0;
      for (int k = 0; k < LR_STATS; k++)
        if (a.has_trg[k]) loss = loss + lr_target_term(st[k], a.trg_lo[k], a.trg_hi[k], a.weight[k]);
      a.loss[lvl] = loss;
    }
    if (a.play) {
      int32_t *p = a.play + (size_t)lvl * 4;
      p[0] = r.searched, p[1] = r.row, p[2] = r.col, p[3] = r.collected;
    }
    if (a.error) a.error[lvl] = err;
  }
}

// lr_evaluate_level's hook for one level (see LrNoHook for the calls): the level's rows of the outputs, the tour's length so
// far (uniform) and what this lane's search of the round left.
struct LrRouteHook {
  int16_t *coords;
  int8_t *moves;
  int32_t *gold_off;
  int16_t *gold_back;
  int32_t gold_cap, route_cap, W, n_cells;
  int32_t tour;                         // cells of the tour so far; the same in every lane
  int32_t off, goal, goal_parent, len;  // this lane's route of the round: off < 0 = none to store

  __device__ __forceinline__ void round_begin() { off = -1, len = 0; }
  __device__ __forceinline__ void searched(int goal_, int goal_parent_, int len_) { goal = goal_, goal_parent = goal_parent_, len = len_; }
  __device__ __forceinline__ void counted(int q, int j, int len_out, int len_back) {
    const int lane = threadIdx.x & 63;
    if ((lane >> 1) == q) off = tour + ((lane & 1) ? len_out : 0);
    if (lane == 0 && j < gold_cap) {
      if (gold_off) gold_off[j] = tour;
      if (gold_back) gold_back[j] = (int16_t)len_back;
    }
    tour += len_out + len_back;
  }
  // cell k of the route at off + k, walking the chain from the goal backwards; `next` is the cell behind `cell` on the route
  __device__ __forceinline__ void round_end(const uint32_t *cells) {
    if (off < 0 || off >= route_cap) return;
    int cell = goal, next = -1, p = goal_parent;
    for (int k = len - 1; k >= 0; k--) {
      const int idx = off + k;
      if (idx < route_cap) {
        if (coords) coords[2 * idx] = (int16_t)(cell / W), coords[2 * idx + 1] = (int16_t)(cell % W);
        if (moves) moves[idx] = next < 0 ? (int8_t)-1 : (int8_t)lr_move_between(cell, next, W);
      }
      if (k == 0 || p < 0 || p >= n_cells) break;  // (the chain has len - 1 parents: the last two cannot happen)
      next = cell, cell = p;
      p = cells[p * 64] & 511u;
    }
  }
};

__global__ __launch_bounds__(64) void loderunner_routes_kernel(const LrRouteArgs a) {
  __shared__ LrLds L;
  const int lane = threadIdx.x;
  const int H = a.lr.h, W = a.lr.w, n_cells = H * W;
  uint32_t *slot = a.lr.ws + (size_t)blockIdx.x * (size_t)(a.lr.ws_stride / 4);
  for (int lvl = blockIdx.x; lvl < a.lr.n; lvl += gridDim.x) {
    const uint8_t *g = a.lr.grids + (size_t)lvl * n_cells;
    bool bad = false;
    for (int i = lane; i < n_cells; i += 64) L.map[i] = lr_tile(g[i], bad);
    const uint32_t err = __any(bad) ? 1u : 0u;
    __syncthreads();
    LrRouteHook hook;
    hook.coords = a.coords ? a.coords + (size_t)lvl * a.route_cap * 2 : nullptr;
    hook.moves = a.moves ? a.moves + (size_t)lvl * a.route_cap : nullptr;
    hook.gold_off = a.gold_off ? a.gold_off + (size_t)lvl * a.lr.gold_cap : nullptr;
    hook.gold_back = a.gold_back ? a.gold_back + (size_t)lvl * a.lr.gold_cap : nullptr;
    hook.gold_cap = a.lr.gold_cap, hook.route_cap = a.route_cap, hook.W = W, hook.n_cells = n_cells;
    hook.tour = 0, hook.off = -1, hook.goal = 0, hook.goal_parent = -1, hook.len = 0;
    LrResult r;
    lr_evaluate_level(L, H, W, slot, r, hook);
    __syncthreads();
    lr_store_level(a.lr, L, r, lvl, err);
    // the golds without a route (the hook stored those with one), and what lies behind the tour
    for (int j = lane; j < a.lr.gold_cap; j += 64)
      if (j >= r.gold || L.state[L.golds[j]] != 1) {
        if (hook.gold_off) hook.gold_off[j] = -1;
        if (hook.gold_back) hook.gold_back[j] = 0;
      }
    for (int k = hook.tour + lane; k < a.route_cap; k += 64) {
      if (hook.coords) hook.coords[2 * k] = -1, hook.coords[2 * k + 1] = -1;
      if (hook.moves) hook.moves[k] = -1;
    }
    if (lane == 0 && a.tour_len) a.tour_len[lvl] = hook.tour;
    __syncthreads();  // the next level's staging overwrites L
  }
}

#endif  // PCGRL_KERNEL_TU

}  // namespace pcgrl
