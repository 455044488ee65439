// loderunner/pcgrl_loderunner.h -- Lode Runner levels on the device (include/pcgrl_amd_loderunner.h): what
// LoderunnerProblem.get_stats computes for an H x W map of 8 tile types (envs/probs/loderunner_prob.py:78-91) -- three tile
// counts and the gold searches of loderunner/engine.py:get_score with its wall clock stopped -- and the loss
// ControlWrapper.get_loss would derive from them.  DESIGN.md section 26 has the rules with every quirk;
// tests/loderunner_rules.py is the same in plain Python.
//
// loderunner_kernel: one 64-lane wave per level, the grid striding over the levels (at most lr_blocks() blocks, so the
// workspace is bounded whatever n).
//   map       the level's bytes are staged in LDS (ids above 7 become 0 and raise error bit 0); lr_evaluate_level takes that
//             LDS map, so a later env kernel can call it on the map it already holds.
//   start     every lane walks the player's fall (uniform); the landing cell becomes empty in LDS.
//   moves     all lanes: one byte per cell, bit m = move m (left right up down d-left d-right) leaves the cell, bits 6-7 =
//             which of the engine's three listing orders the cell's branch uses.  A function of the level alone, so both
//             searches of every gold read it.
//   searches  the 2 G searches of a level are pure functions of (level, source, goal): one search per lane, 32 golds (to the
//             gold in the even lane, back to the start in the odd one) per round.  A gold already collected when its round
//             starts is not searched.  The open list is an array of FIFO buckets indexed by score (Manhattan distance + steps
//             <= H + W + H W): the engine orders by (score, insertion counter), the counter is unique, and a FIFO keeps counter
//             order, so "head of the lowest non-empty bucket" is the engine's heappop exactly.  The heuristic is inconsistent
//             (a diagonal fall covers two Manhattan units in a step), so a push may lower the minimum: by one at most.
//   memory    per block a workspace slot in HBM, lane-interleaved (word i of lane l at i * 64 + l): per lane 4 H W + 1 nodes
//             (cell 9 | parent cell 9 | next in bucket 12), H + W + H W + 1 buckets (head 16 | tail 16) and H W cells (closed 1 |
//             parent cell 9).  A search expands a cell once and an expansion pushes at most 4 children, which bounds the
//             nodes; buckets and cells are cleared by the search that reads them and nodes are written before they are read,
//             so a dirty workspace does not matter.
//   paths     a cell is expanded once, so "the node expanded at the parent's cell" is the parent node: the chain of parent
//             cells is the path.  Each lane marks its path's parents in a 512-bit LDS row.
//   golds     sequential over the round's golds in row-major order, all lanes on the cells: the skip rule, the first search's
//             node count into path-length, and every unfound gold on a marked cell of either path becomes found.
//   hooks     lr_evaluate_level takes a hook object (LrNoHook: nothing) that is told of every search, of every pair that counts
//             and of the end of every round: how loderunner_routes_kernel (pcgrl_loderunner_routes.h) reads the routes out of
//             the parent chains without a second copy of the search or of the accumulation.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcgrl {

constexpr int LR_TILES = 8;
constexpr int LR_STATS = 5;  // player, enemies, gold, win, path-length
constexpr int LR_MAX_H = 16, LR_MAX_W = 32, LR_MAX_CELLS = LR_MAX_H * LR_MAX_W;
// blocks per launch: as many as fit LR_WS_BUDGET bytes of workspace, between LR_MIN_BLOCKS (one wave per CU) and LR_MAX_BLOCKS
// (four per SIMD on 256 CUs); measured at 8 x 12, 4 096 blocks take 0.55 x the time of 1 024
#ifndef PCGRL_LR_MAX_BLOCKS  // (a development build with another value: _lib.build(out=..., defines=("PCGRL_LR_MAX_BLOCKS=1024",)))
#define PCGRL_LR_MAX_BLOCKS 4096
#endif
constexpr int LR_MIN_BLOCKS = 256, LR_MAX_BLOCKS = PCGRL_LR_MAX_BLOCKS;
constexpr int64_t LR_WS_BUDGET = 640ll << 20;
constexpr int LR_EMPTY = 0, LR_BRICK = 1, LR_LADDER = 2, LR_ROPE = 3, LR_SOLID = 4, LR_GOLD = 5, LR_ENEMY = 6, LR_PLAYER = 7;
constexpr uint32_t LR_NIL = 0xFFFu, LR_NO_BUCKET = 0xFFFFFFFFu, LR_CLOSED = 0x8000u;

struct LrArgs {
  int32_t h, w, n;
  const uint8_t *grids;  // uint8 [n][h][w]
  uint32_t *ws;          // gridDim.x slots of ws_stride bytes
  int64_t ws_stride;
  int32_t gold_cap;
  double *stats;         // [n][5]
  double *loss;          // [n] or null
  int32_t *play;         // [n][4] or null
  int8_t *gold_state;    // [n][gold_cap] or null
  int16_t *gold_dist;    // [n][gold_cap] or null
  uint32_t *error;       // [n] or null
  int32_t has_trg[LR_STATS];
  double weight[LR_STATS], trg_lo[LR_STATS], trg_hi[LR_STATS];
};

__host__ __device__ inline int lr_nodes(int cells) { return 4 * cells + 1; }
__host__ __device__ inline int lr_scores(int h, int w) { return h + w + h * w + 1; }
// one block's workspace slot: 64 lanes of nodes, buckets and cells, 4 bytes each
inline int64_t lr_ws_stride(int h, int w) { return (int64_t)(lr_nodes(h * w) + lr_scores(h, w) + h * w) * 64 * 4; }
inline int lr_blocks(int n, int h, int w) {
  const int64_t fit = LR_WS_BUDGET / lr_ws_stride(h, w);
  const int cap = fit < LR_MIN_BLOCKS ? LR_MIN_BLOCKS : (fit > LR_MAX_BLOCKS ? LR_MAX_BLOCKS : (int)fit);
  return n < cap ? n : cap;
}

hipError_t launch_loderunner(const LrArgs &a, hipStream_t s);

#ifdef PCGRL_KERNEL_TU

struct LrLds {
  uint8_t map[LR_MAX_CELLS];     // tile ids; the landing cell already empty
  uint8_t moves[LR_MAX_CELLS];   // bits 0-5 the moves, bits 6-7 the listing order
  uint8_t state[LR_MAX_CELLS];   // per gold cell: 0 not collected, 1 own searches, 2 another gold's path, 3 the fall
  uint16_t dist[LR_MAX_CELLS];   // per gold cell: what it added to path-length
  uint16_t golds[LR_MAX_CELLS];  // the gold cells in row-major order
  uint32_t marks[LR_MAX_CELLS / 32][64];  // per lane (the fast index: no bank conflicts): the parent cells of its path
  uint16_t len[64];              // per lane: nodes on its path, 0 = no path
};

// what one level's evaluation leaves (every lane holds the same values)
struct LrResult {
  int32_t player, enemies, gold;
  double win;
  int32_t path_length, searched, row, col, collected;
};

// a map byte as the kernels read it: a tile id above 7 reads as empty and sets `bad` (the caller raises its error bit)
__device__ __forceinline__ uint8_t lr_tile(uint8_t t, bool &bad) {
  if (t >= LR_TILES) {
    bad = true;
    return 0;
  }
  return t;
}

// One term of the loss: -(distance of the statistic to its zero-loss interval [lo, hi]) * weight, rounded to double before it
// is added (no fused multiply-add): the Python rules bit for bit.
__device__ __forceinline__ double lr_target_term(double v, double lo, double hi, double weight) {
#pragma clang fp contract(off)
  const double d = v < lo ? lo - v : (v > hi ? v - hi : 0.0);
  return -d * weight;
}

__device__ __forceinline__ bool lr_block(int t) { return t == LR_BRICK || t == LR_SOLID; }
__device__ __forceinline__ bool lr_support(int t) { return t == LR_BRICK || t == LR_SOLID || t == LR_LADDER; }
__device__ __forceinline__ bool lr_free(int t) { return t == LR_GOLD || t == LR_ENEMY || t == LR_EMPTY; }
__device__ __forceinline__ bool lr_hang(int t) { return t == LR_LADDER || t == LR_ROPE; }

// Node.get_actions (loderunner/engine.py:52-165) for one cell: bits 0-5 = left right up down d-left d-right, bits 6-7 = the
// order the branch lists them in (0: L R U D DL DR; 1, a ladder above the bottom row: U D L R DL DR; 2, a rope above the
// bottom row: D L R DL DR).  Brick, solid and the left-behind player have no moves.
__device__ inline uint32_t lr_cell_moves(const uint8_t *map, int H, int W, int r, int c) {
  const int t = map[r * W + c];
  const bool bottom = r == H - 1;
  uint32_t m = 0;
  if (t != LR_LADDER && t != LR_ROPE && !lr_free(t)) return 0;
  if (bottom) {
    if (c > 0 && !lr_block(map[r * W + c - 1])) m |= 1u;
    if (c < W - 1 && !lr_block(map[r * W + c + 1])) m |= 2u;
    if (t == LR_LADDER && r > 0 && !lr_block(map[(r - 1) * W + c])) m |= 4u;
    return m;
  }
  const int below = map[(r + 1) * W + c];
  uint32_t side = 0;  // what a cell that stands, climbs or hangs may do sideways
  if (c > 0) {
    const int s = map[r * W + c - 1], sb = map[(r + 1) * W + c - 1];
    if (lr_hang(s) || (lr_free(s) && lr_support(sb))) side |= 1u;
    if (lr_free(s) && !lr_support(sb)) side |= 16u;
  }
  if (c < W - 1) {
    const int s = map[r * W + c + 1], sb = map[(r + 1) * W + c + 1];
    if (lr_hang(s) || (lr_free(s) && lr_support(sb))) side |= 2u;
    if (lr_free(s) && !lr_support(sb)) side |= 32u;
  }
  if (t == LR_LADDER) {
    if (r > 0 && !lr_block(map[(r - 1) * W + c])) m |= 4u;
    if (!lr_block(below)) m |= 8u;
    return m | side | (1u << 6);
  }
  if (t == LR_ROPE) {
    if (!lr_block(below)) m |= 8u;
    return m | side | (2u << 6);
  }
  if (!lr_support(below)) return 8u;  // falling: nothing else
  if (below == LR_LADDER) m |= 8u;
  return m | side;
}

// a listing order: six 3-bit move numbers, the first in the low bits (a rope's order never has `up`)
__host__ __device__ constexpr uint32_t lr_order(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e, uint32_t f) {
  return a | (b << 3) | (c << 6) | (d << 9) | (e << 12) | (f << 15);
}

// AStar.run (engine.py:244-269) from cell `src` to cell `goal`, by one lane on its own workspace words (word i at p[i * 64]).
// Returns the nodes on the path found (steps + 1), 0 when the open list empties; marks the path's parent cells in `marks`
// (bit p of the lane's row: word p / 32 at marks[(p / 32) * 64]).  The goal is never closed, so its parent leaves in
// `goal_parent` (-1 when the root is the goal); the parents before it stay in `cells` until the lane's next search.
__device__ inline int lr_search(const LrLds &L, int H, int W, int src, int goal, uint32_t *nodes, uint32_t *buckets, uint32_t *cells,
                                uint32_t *marks, int &goal_parent) {
  const int n_cells = H * W, n_scores = lr_scores(H, W), max_nodes = lr_nodes(n_cells);
  const int gr = goal / W, gc = goal % W;
  for (int i = 0; i < n_cells; i++) cells[i * 64] = 0;
  for (int i = 0; i < n_scores; i++) buckets[i * 64] = LR_NO_BUCKET;
  int cur = abs(src / W - gr) + abs(src % W - gc);
  nodes[0] = (uint32_t)src | ((uint32_t)src << 9) | (LR_NIL << 18);
  buckets[cur * 64] = 0;  // head 0, tail 0
  int cnt = 0, open = 1;
  while (open > 0) {
    while (cur < n_scores - 1 && buckets[cur * 64] == LR_NO_BUCKET) cur++;
    const uint32_t b = buckets[cur * 64];
    if (b == LR_NO_BUCKET) return 0;  // (cannot happen while open > 0)
    const uint32_t head = b & 0xFFFFu, nd = nodes[head * 64], next = nd >> 18;
    buckets[cur * 64] = next == LR_NIL ? LR_NO_BUCKET : ((b & 0xFFFF0000u) | next);
    open--;
    const int cell = nd & 511u, parent = (nd >> 9) & 511u;
    if (cells[cell * 64] & LR_CLOSED) continue;
    if (cell == goal) {
      goal_parent = head != 0 ? parent : -1;
      if (head != 0) {  // the root as the goal has no parents
        int p = parent;
        for (int guard = 0; guard < n_cells; guard++) {
          marks[(p >> 5) * 64] |= 1u << (p & 31);
          if (p == src) break;
          p = cells[p * 64] & 511u;
        }
      }
      return cur + 1;  // the Manhattan part is 0 here: score = steps
    }
    cells[cell * 64] = LR_CLOSED | (uint32_t)parent;
    const int r = cell / W, c = cell % W;
    const int step1 = cur - (abs(r - gr) + abs(c - gc)) + 1;
    const uint32_t mv = L.moves[cell];
    const uint32_t order = (mv >> 6) == 0 ? lr_order(0, 1, 2, 3, 4, 5) : ((mv >> 6) == 1 ? lr_order(2, 3, 0, 1, 4, 5) : lr_order(3, 0, 1, 2, 4, 5));
    for (int k = 0; k < 6; k++) {
      const int m = (order >> (3 * k)) & 7;
      if (!((mv >> m) & 1u)) continue;
      const int cr = r + (m == 2 ? -1 : (m >= 3 ? 1 : 0)), cc = c + ((m == 0 || m == 4) ? -1 : ((m == 1 || m == 5) ? 1 : 0));
      const int s = abs(cr - gr) + abs(cc - gc) + step1;
      if (cnt + 1 >= max_nodes || s >= n_scores) return 0;  // (cannot happen: 4 pushes per cell, a cell expanded once)
      cnt++;
      nodes[cnt * 64] = (uint32_t)(cr * W + cc) | ((uint32_t)cell << 9) | (LR_NIL << 18);
      const uint32_t sb = buckets[s * 64];
      if (sb == LR_NO_BUCKET) {
        buckets[s * 64] = (uint32_t)cnt | ((uint32_t)cnt << 16);
      } else {
        const uint32_t tail = sb >> 16;
        nodes[tail * 64] = (nodes[tail * 64] & 0x3FFFFu) | ((uint32_t)cnt << 18);
        buckets[s * 64] = (sb & 0xFFFFu) | ((uint32_t)cnt << 16);
      }
      open++;
      cur = min(cur, s);
    }
  }
  return 0;
}

// The hook of lr_evaluate_level that does nothing.  A hook's calls: round_begin by every lane before a round's searches;
// searched by the lane that ran a search (its goal, the goal's parent, the nodes on the path, 0 = none); counted by every lane,
// in gold order, for gold j (pair q of its round) whose pair of searches counts, with the nodes of its two paths; round_end
// by every lane after the round's accumulation, while the lane's parent chain in `cells` still stands.
struct LrNoHook {
  __device__ __forceinline__ void round_begin() {}
  __device__ __forceinline__ void searched(int, int, int) {}
  __device__ __forceinline__ void counted(int, int, int, int) {}
  __device__ __forceinline__ void round_end(const uint32_t *) {}
};

// One level, by one 64-lane wave: the statistics and the gold record of the map in L.map ([H][W], ids 0..7; the landing cell
// is overwritten).  slot: this block's workspace.  L.state / L.dist / L.golds hold the per-gold record afterwards, r.gold
// entries.  Every lane returns with the same LrResult.  For a block of exactly one 64-lane wave: the lane id is wave-local, the
// barriers are block-wide and the LDS rows are indexed by lane, so a kernel with more waves per block must not call it as it is.
template <class Hook>
__device__ inline void lr_evaluate_level(LrLds &L, int H, int W, uint32_t *slot, LrResult &r, Hook &hook) {
  const int lane = threadIdx.x & 63, n_cells = H * W;
  // counts, the player's cell, the gold list in row-major order
  int players = 0, enemies = 0, golds = 0, pcell = -1;
  for (int base = 0; base < n_cells; base += 64) {
    const int i = base + lane;
    const int t = i < n_cells ? L.map[i] : -1;
    const uint64_t gm = __ballot(t == LR_GOLD), pm = __ballot(t == LR_PLAYER);
    if (t == LR_GOLD) L.golds[golds + __popcll(gm & ((1ull << lane) - 1))] = (uint16_t)i;
    if (i < n_cells) {
      L.state[i] = 0;
      L.dist[i] = 0;
    }
    golds += __popcll(gm);
    players += __popcll(pm);
    enemies += __popcll(__ballot(t == LR_ENEMY));
    if (pm && pcell < 0) pcell = base + __ffsll((unsigned long long)pm) - 1;
  }
  r.player = players, r.enemies = enemies, r.gold = golds;
  r.win = 0.0;
  r.path_length = 0, r.searched = 0, r.row = -1, r.col = -1, r.collected = 0;
  __syncthreads();
  if (players != 1) return;  // nothing is searched (loderunner_prob.py:88)
  // get_starting_point (engine.py:323-338): the fall, uniform over the lanes
  int row = pcell / W;
  const int col = pcell % W;
  int collected = 0;
  while (row != H - 1 && !lr_support(L.map[(row + 1) * W + col]) && L.map[row * W + col] != LR_ROPE) {
    row++;
    if (L.map[row * W + col] == LR_GOLD) {
      collected++;
      if (lane == 0) L.state[row * W + col] = 3;
    }
  }
  const int start = row * W + col;
  r.searched = 1, r.row = row, r.col = col;
  __syncthreads();
  if (lane == 0) L.map[start] = LR_EMPTY;  // (the player's own cell keeps its M when the player fell)
  __syncthreads();
  if (golds == 0) {
    r.win = -1.0;
    return;
  }
  for (int i = lane; i < n_cells; i += 64) L.moves[i] = (uint8_t)lr_cell_moves(L.map, H, W, i / W, i % W);
  __syncthreads();
  uint32_t *nodes = slot + lane, *buckets = nodes + (size_t)lr_nodes(n_cells) * 64, *cells = buckets + (size_t)lr_scores(H, W) * 64;
  int total = 0;
  for (int base = 0; base < golds; base += 32) {
    const int j = base + (lane >> 1);
    for (int k = 0; k < (n_cells + 31) / 32; k++) L.marks[k][lane] = 0;
    int len = 0;
    hook.round_begin();
    if (j < golds && L.state[L.golds[j]] == 0) {
      // source and goal are picked per lane and the search is called once, so the outward and the return searches of the round
      // run in the same instructions, side by side
      const int g = L.golds[j];
      const int src = (lane & 1) ? g : start, goal = (lane & 1) ? start : g;
      int goal_parent = -1;
      len = lr_search(L, H, W, src, goal, nodes, buckets, cells, &L.marks[0][lane], goal_parent);
      hook.searched(goal, goal_parent, len);
    }
    L.len[lane] = (uint16_t)len;
    __syncthreads();
    // find_all_golds (engine.py:281-308): the accumulation over this round's golds, in order
    const int round = min(32, golds - base);
    for (int q = 0; q < round; q++) {
      const int g = L.golds[base + q];
      const bool counts = L.state[g] == 0 && L.len[2 * q] != 0 && L.len[2 * q + 1] != 0;
      __syncthreads();
      if (counts) {
        hook.counted(q, base + q, L.len[2 * q], L.len[2 * q + 1]);
        total += L.len[2 * q];
        for (int i = lane; i < n_cells; i += 64) {
          const uint32_t bit = (L.marks[i >> 5][2 * q] | L.marks[i >> 5][2 * q + 1]) >> (i & 31);
          if ((bit & 1u) && L.map[i] == LR_GOLD && L.state[i] == 0 && i != g) L.state[i] = 2;
        }
        if (lane == 0) {
          L.state[g] = 1;
          L.dist[g] = L.len[2 * q];
        }
      }
      __syncthreads();
    }
    hook.round_end(cells);
  }
  int found = 0;
  for (int base = 0; base < golds; base += 64) {
    const int j = base + lane;
    found += __popcll(__ballot(j < golds && (L.state[L.golds[j]] == 1 || L.state[L.golds[j]] == 2)));
  }
  collected += found;
  r.collected = collected;
  r.path_length = total;
  r.win = 1.0 / (double)(1 + (golds - collected));
}

__device__ inline void lr_evaluate_level(LrLds &L, int H, int W, uint32_t *slot, LrResult &r) {
  LrNoHook none;
  lr_evaluate_level(L, H, W, slot, r, none);
}

#ifndef PCGRL_LR_DEVICE_ONLY  // (loderunner_routes_kernel takes the device functions above without a second loderunner_kernel)
__global__ __launch_bounds__(64) void loderunner_kernel(const LrArgs a) {
  __shared__ LrLds L;
  const int lane = threadIdx.x;
  const int H = a.h, W = a.w, n_cells = H * W;
  uint32_t *slot = a.ws + (size_t)blockIdx.x * (size_t)(a.ws_stride / 4);
  for (int lvl = blockIdx.x; lvl < a.n; lvl += gridDim.x) {
    const uint8_t *g = a.grids + (size_t)lvl * n_cells;
    bool bad = false;
    for (int i = lane; i < n_cells; i += 64) L.map[i] = lr_tile(g[i], bad);
    const uint32_t err = __any(bad) ? 1u : 0u;
    __syncthreads();
    LrResult r;
    lr_evaluate_level(L, H, W, slot, r);
    __syncthreads();
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
    __syncthreads();  // the next level's staging overwrites L
  }
}
#endif  // PCGRL_LR_DEVICE_ONLY

#endif  // PCGRL_KERNEL_TU

}  // namespace pcgrl
