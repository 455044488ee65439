// ddave/pcgrl_ddave.h -- Dangerous Dave levels on the device (include/pcgrl_amd_ddave.h): what DDaveProblem.get_stats computes
// for an H x W map of 7 tile types (envs/probs/ddave/ddave_prob.py:149-169) -- seven map statistics and the four-stage
// play-through of ddave/engine.py.  DESIGN.md section 31 has the rules with every quirk; tests/ddave_rules.py is the same in
// plain Python.
//
// ddave_kernel: one 64-lane wave per level.
//   map       the level's bytes are staged in LDS with byte loads (any alignment; an id above 6 becomes solid and raises error
//             bit 0).
//   scans     lane-parallel: a lane counts the tiles of cells lane, lane + 64, ... and walks down from each player tile for
//             dist-floor; wave reductions.  Lane r < H then builds row r's masks (passable, solid, spike) and its diamonds'
//             row-major ordinals; the regions are peeled off one at a time, a row per lane, the flood's neighbour rows taken by
//             shuffles (every loop bounded by the cell count).
//   level     in LDS, with the solid border: solid[y] and spike[y] bit rows (y < H + 2 <= 18, x < W + 2 <= 34), ord[y][x] the
//             diamond ordinal of a cell (255: none); the player, key and door positions in registers.
//   search    lane 0 alone, as smb_search (smb/pcgrl_smb.h has the reasons): the cost of an iteration is the chain of dependent
//             loads of the heap's sifts and of the hash probe, hidden by occupancy.  The A* open list is CPython's heapq
//             (dd_heap_push / dd_heap_pop are smb_heap_push / smb_heap_pop with a 16-bit node index), ordered with `<` alone by
//             f = 2 * heuristic + (2 * balance) * depth + DD_F_BIAS, an exact integer image of heuristic + balance * depth
//             that is never negative.  The BFS pops in push order, which is the order of the node array: its open list is an
//             index into it.
//   memory    per level a workspace slot in HBM: nodes (16 B: x 6 | y 5 | airTime 2 | col_key 1 | lost 1 | action 2 | jumps 14 ;
//             parent 16 | depth 14 ; the 64-bit set of diamonds still on the map), 4 * power + 1 of them -- an expansion pushes
//             four and there are at most `power` expansions -- reused by the next stage; the heap (4 B: f 16 | node 16), as
//             many; the visited set, open-addressed with linear probing over C >= 2 * power slots (a 32-bit tag: x, y,
//             col_key and an occupied bit; the 64-bit diamond set beside it), whose tags the whole wave clears before each
//             stage.  At most `power` keys are inserted, so a probe meets a free slot within C steps.  Nodes and heap are
//             written before they are read, so a dirty workspace does not matter.
//   outputs   the returned node's parent chain gives the moves (lane 0); all lanes fill the tail with -1.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../measures/pcgrl_measures_wave.h"  // MeasWaveArgs, meas_wave_map

namespace pcgrl {

constexpr int DD_TILES = 7;
constexpr int DD_STATS = 11;  // player, dist-floor, exit, diamonds, key, spikes, regions, num-jumps, col-diamonds, dist-win, sol-length
constexpr int DD_PLAY = 12;
constexpr int DD_MAX_H = 16, DD_MAX_W = 32;
constexpr int DD_MAX_CELLS = DD_MAX_H * DD_MAX_W;  // 512
constexpr int DD_MAX_POWER = 16000;   // depth, jumps < 2^14; 4 * power + 1 nodes < 2^16
constexpr int DD_MAX_DIAMONDS = 64;   // the remaining diamonds are one 64-bit word
constexpr int DD_LW = DD_MAX_W + 2, DD_LH = DD_MAX_H + 2;
// 2 * heuristic >= -2 * 5 * 64; 2 * heuristic + 2 * depth + bias <= 2 * (31 + 15 + 52) + 32 000 + 640 < 2^16
constexpr int DD_F_BIAS = 2 * 5 * DD_MAX_DIAMONDS;
constexpr int DD_MEAS_TILES = 7, DD_MEAS_PLANES = 3;

struct DdArgs {
  int32_t h, w, power, n;
  const uint8_t *grids;  // uint8 [n][h][w]
  uint8_t *ws;           // n slots of ws_stride bytes, 16-byte aligned
  int64_t ws_stride;
  int32_t hash_cap;      // a power of two, >= 2 * power and >= 16
  int32_t cap;
  int32_t *stats;        // [n][11]
  int8_t *moves;         // [n][cap] or null
  int32_t *length;       // [n] or null
  int32_t *play;         // [n][12] or null
  uint32_t *error;       // [n] or null
};

__host__ __device__ inline int64_t dd_nodes_per_stage(int power) { return 4 * (int64_t)power + 1; }
inline int32_t dd_hash_cap(int power) {
  int32_t c = 16;
  while (c < 2 * power) c <<= 1;
  return c;
}
__host__ __device__ inline int64_t dd_heap_bytes(int power) { return (dd_nodes_per_stage(power) * 4 + 15) / 16 * 16; }
// one level's workspace slot: the nodes, the visited set's diamond words, its tags, the heap; a multiple of 16 bytes
inline int64_t dd_ws_stride(int power) {
  return dd_nodes_per_stage(power) * 16 + (int64_t)dd_hash_cap(power) * 12 + dd_heap_bytes(power);
}

hipError_t launch_ddave(const DdArgs &a, hipStream_t s);
hipError_t launch_dd_measures(const MeasWaveArgs &a, hipStream_t s);

#ifdef PCGRL_DD_KERNEL  // (ddave/pcgrl_k_ddave.hip has it)

struct DdLds {
  uint8_t map[DD_MAX_CELLS];
  uint64_t solid[DD_LH], spike[DD_LH];
  uint8_t ord[DD_LH * DD_LW];
};

// what the search reads besides the LDS level (lane 0's registers)
struct DdGame {
  int px, py, kx, ky, dx, dy;  // bordered coordinates
  int wh;                      // (W + 2) + (H + 2): State.width + State.height
  int nd;                      // diamonds in the level, <= 64
};

__device__ __forceinline__ int dd_wave_sum(int v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int dd_wave_max(int v) {
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ uint32_t dd_key(uint32_t e) { return e >> 16; }

// heapq.heappush: the item goes to the end, then _siftdown(heap, 0, n - 1)
__device__ __forceinline__ void dd_heap_push(uint32_t *heap, int &n, uint32_t item) {
  int pos = n++;
  while (pos > 0) {
    const int pp = (pos - 1) >> 1;
    const uint32_t parent = heap[pp];
    if (!(dd_key(item) < dd_key(parent))) break;
    heap[pos] = parent;
    pos = pp;
  }
  heap[pos] = item;
}

// heapq.heappop: the last item replaces the root, _siftup(heap, 0)
__device__ __forceinline__ uint32_t dd_heap_pop(uint32_t *heap, int &n) {
  const uint32_t last = heap[--n];
  if (n == 0) return last;
  const uint32_t ret = heap[0];
  int pos = 0, child = 1;
  while (child < n) {  // bubble the smaller child up until a leaf
    uint32_t c = heap[child];
    if (child + 1 < n) {
      const uint32_t r = heap[child + 1];
      if (!(dd_key(c) < dd_key(r))) {
        c = r;
        child++;
      }
    }
    heap[pos] = c;
    pos = child;
    child = 2 * pos + 1;
  }
  while (pos > 0) {  // _siftdown(heap, 0, pos) of the item that was last
    const int pp = (pos - 1) >> 1;
    const uint32_t parent = heap[pp];
    if (!(dd_key(last) < dd_key(parent))) break;
    heap[pos] = parent;
    pos = pp;
  }
  heap[pos] = last;
  return ret;
}

__device__ __forceinline__ uint4 dd_pack(int x, int y, int air, int key, int lost, int action, int jumps, uint32_t parent,
                                         int depth, uint64_t left) {
  return make_uint4((uint32_t)x | ((uint32_t)y << 6) | ((uint32_t)air << 11) | ((uint32_t)key << 13) | ((uint32_t)lost << 14) |
                        ((uint32_t)action << 15) | ((uint32_t)jumps << 17),
                    parent | ((uint32_t)depth << 16), (uint32_t)left, (uint32_t)(left >> 32));
}
__device__ __forceinline__ int dd_nx(uint4 v) { return v.x & 0x3F; }
__device__ __forceinline__ int dd_ny(uint4 v) { return (v.x >> 6) & 0x1F; }
__device__ __forceinline__ int dd_nair(uint4 v) { return (v.x >> 11) & 3; }
__device__ __forceinline__ int dd_nkey(uint4 v) { return (v.x >> 13) & 1; }
__device__ __forceinline__ int dd_nlost(uint4 v) { return (v.x >> 14) & 1; }
__device__ __forceinline__ int dd_naction(uint4 v) { return (v.x >> 15) & 3; }
__device__ __forceinline__ int dd_njumps(uint4 v) { return (v.x >> 17) & 0x3FFF; }
__device__ __forceinline__ uint32_t dd_nparent(uint4 v) { return v.y & 0xFFFFu; }
__device__ __forceinline__ int dd_ndepth(uint4 v) { return (v.y >> 16) & 0x3FFF; }
__device__ __forceinline__ uint64_t dd_nleft(uint4 v) { return (uint64_t)v.z | ((uint64_t)v.w << 32); }

// State.getHeuristic (engine.py:278-283)
__device__ __forceinline__ int dd_heuristic(const DdGame &g, int x, int y, int key, uint64_t left) {
  const int dist = key ? abs(x - g.dx) + abs(y - g.dy) : abs(x - g.kx) + abs(y - g.ky) + g.wh;
  return dist - 5 * (g.nd - __popcll(left));
}

__device__ __forceinline__ bool dd_solid(const DdLds &L, int x, int y) { return (L.solid[y] >> x) & 1u; }

// The visited set: true when (tag, left) is in it, else it goes in.  At most `power` <= C / 2 keys are ever inserted, so the
// probe ends at a free slot; the bound is for the compiler's and the reader's peace.
__device__ __forceinline__ bool dd_visited(uint32_t *tags, uint64_t *lefts, uint32_t capmask, uint32_t tag, uint64_t left) {
  uint32_t h = tag * 0xC2B2AE3Du ^ (uint32_t)left * 0x9E3779B1u ^ (uint32_t)(left >> 32) * 0x85EBCA77u;
  h ^= h >> 15;
  uint32_t i = h & capmask;
  for (uint32_t probe = 0; probe <= capmask; probe++) {
    const uint32_t t = tags[i];
    if (t == 0) {
      tags[i] = tag;
      lefts[i] = left;
      return false;
    }
    if (t == tag && lefts[i] == left) return true;
    i = (i + 1) & capmask;
  }
  return false;
}

// One of the four searches (one lane): AStarAgent.getSolution with balance2 / 2 (engine.py:105-129), or BFSAgent.getSolution
// when balance2 < 0 (engine.py:61-81).  Returns the node it ends on -- the winner, else the best node -- and the iterations it
// ran.  The tags must be zero on entry.
__device__ inline uint32_t dd_search(const DdLds &L, const DdGame &g, uint4 *nodes, uint32_t *heap, uint32_t *tags, uint64_t *lefts,
                                     uint32_t capmask, int power, int balance2, int &iterations, bool &won) {
  const bool astar = balance2 >= 0;
  const uint64_t all = g.nd >= 64 ? ~0ull : (1ull << g.nd) - 1ull;
  nodes[0] = dd_pack(g.px, g.py, 0, 0, 0, 0, 0, 0, 0, all);
  int nn = 1, hn = 0, head = 0, it = 0;
  if (astar) {
    heap[0] = (uint32_t)(2 * dd_heuristic(g, g.px, g.py, 0, all) + DD_F_BIAS) << 16;
    hn = 1;
  }
  uint32_t best = 0;
  int best_h = 0x7FFFFFFF, best_depth = 0;
  won = false;
  while (it < power && (astar ? hn > 0 : head < nn)) {
    it++;
    const uint32_t cur = astar ? (dd_heap_pop(heap, hn) & 0xFFFFu) : (uint32_t)head++;
    const uint4 nd = nodes[cur];
    if (dd_nlost(nd)) continue;
    const int x = dd_nx(nd), y = dd_ny(nd), air = dd_nair(nd), key = dd_nkey(nd), jumps = dd_njumps(nd), depth = dd_ndepth(nd);
    const uint64_t left = dd_nleft(nd);
    if (key && x == g.dx && y == g.dy) {
      best = cur;
      won = true;
      break;
    }
    if (dd_visited(tags, lefts, capmask, 0x80000000u | (uint32_t)x | ((uint32_t)y << 6) | ((uint32_t)key << 11), left)) continue;
    const int h = dd_heuristic(g, x, y, key, left);
    if (h < best_h || (h == best_h && depth < best_depth)) {
      best = cur;
      best_h = h;
      best_depth = depth;
    }
    // State.update (engine.py:229-264) for directions 0..3 = stay, left, right, jump
    const bool ground = dd_solid(L, x, y + 1), ceiling = dd_solid(L, x, y - 1);
    for (int a = 0; a < 4; a++) {
      int cx = x, cy = y, cair = air, cj = jumps, ckey = key, lost = 0;
      uint64_t cleft = left;
      if (a == 1 || a == 2) {
        const int tx = a == 1 ? x - 1 : x + 1;
        if (!dd_solid(L, tx, y)) cx = tx;
      } else if (a == 3) {
        if (ground && !ceiling) {
          cair = 3;
          cj++;
        }
      }
      if (cair > 1) {
        cair--;
        if (!dd_solid(L, cx, cy - 1)) cy--;
        else cair = 1;
      } else if (cair == 1) {
        cair = 0;
      } else if (!dd_solid(L, cx, cy + 1)) {
        cy++;
      }
      // updatePlayer (engine.py:212-227): a diamond, else a spike, else the key
      const uint32_t o = L.ord[cy * DD_LW + cx];
      if (o < 64 && ((cleft >> o) & 1ull)) cleft &= ~(1ull << o);
      else if ((L.spike[cy] >> cx) & 1u) lost = 1;
      else if (!ckey && cx == g.kx && cy == g.ky) ckey = 1;
      nodes[nn] = dd_pack(cx, cy, cair, ckey, lost, a, cj, cur, depth + 1, cleft);
      if (astar) {
        const int f = 2 * dd_heuristic(g, cx, cy, ckey, cleft) + balance2 * (depth + 1) + DD_F_BIAS;
        dd_heap_push(heap, hn, ((uint32_t)f << 16) | (uint32_t)nn);
      }
      nn++;
    }
  }
  iterations = it;
  return best;
}

__global__ __launch_bounds__(64) void ddave_kernel(const DdArgs a) {
  __shared__ DdLds L;
  const int lvl = blockIdx.x, lane = threadIdx.x;
  if (lvl >= a.n) return;
  const int H = a.h, W = a.w, cells = H * W;
  const uint8_t *grid = a.grids + (size_t)lvl * cells;
  bool bad = false;
  for (int i = lane; i < cells; i += 64) {
    uint8_t t = grid[i];
    if (t >= DD_TILES) {
      bad = true;
      t = 1;
    }
    L.map[i] = t;
  }
  const uint32_t err = __any(bad) ? 1u : 0u;
  __syncthreads();

  // the counts, dist-floor, and where the player, the door and the key are (the last of each; the game needs exactly one)
  int cnt_player = 0, cnt_exit = 0, cnt_diamond = 0, cnt_key = 0, cnt_spike = 0, dist_floor = 0;
  int at_player = -1, at_exit = -1, at_key = -1;
  for (int i = lane; i < cells; i += 64) {
    const int t = L.map[i];
    cnt_exit += t == 3;
    cnt_diamond += t == 4;
    cnt_key += t == 5;
    cnt_spike += t == 6;
    if (t == 3) at_exit = i;
    if (t == 5) at_key = i;
    if (t == 2) {
      cnt_player++;
      at_player = i;
      const int r = i / W, c = i - r * W;
      int d = H - 1;  // _calc_dist_floor (helper.py:40-46): dy - 1 of the first solid below, H - 1 without one
      for (int dy = 1; r + dy < H; dy++)
        if (L.map[(r + dy) * W + c] == 1) {
          d = dy - 1;
          break;
        }
      dist_floor += d;
    }
  }
  int32_t stats[DD_STATS];
  stats[0] = dd_wave_sum(cnt_player);
  stats[1] = dd_wave_sum(dist_floor);
  stats[2] = dd_wave_sum(cnt_exit);
  stats[3] = dd_wave_sum(cnt_diamond);
  stats[4] = dd_wave_sum(cnt_key);
  stats[5] = dd_wave_sum(cnt_spike);
  at_player = dd_wave_max(at_player);
  at_exit = dd_wave_max(at_exit);
  at_key = dd_wave_max(at_key);

  // lane r < H: row r's masks, its diamonds' ordinals, and its rows of the bordered level
  uint32_t pass = 0, solid = 0, spike = 0, dia = 0;
  if (lane < H)
    for (int c = 0; c < W; c++) {
      const int t = L.map[lane * W + c];
      solid |= (uint32_t)(t == 1) << c;
      spike |= (uint32_t)(t == 6) << c;
      dia |= (uint32_t)(t == 4) << c;
    }
  if (lane < H) pass = ~(solid | spike) & (W == 32 ? ~0u : (1u << W) - 1u);
  const int row_dia = __popc(dia);
  int before = 0;  // diamonds in the rows above
  for (int r = 0; r < DD_MAX_H - 1; r++) {
    const int v = __shfl(row_dia, r, 64);
    if (r < lane) before += v;
  }
  if (lane < H) {
    L.solid[lane + 1] = ((uint64_t)solid << 1) | 1ull | (1ull << (W + 1));
    L.spike[lane + 1] = (uint64_t)spike << 1;
    for (int c = 0; c < W; c++) {
      const int o = before + __popc(dia & ((1u << c) - 1u));
      L.ord[(lane + 1) * DD_LW + c + 1] = ((dia >> c) & 1u) ? (uint8_t)min(o, 255) : (uint8_t)255;
    }
  } else if (lane < H + 2) {
    const int y = lane == H ? 0 : H + 1;
    L.solid[y] = (1ull << (W + 2)) - 1ull;
    L.spike[y] = 0;
  }

  // calc_num_regions (helper.py:200-210) over everything but solid and spike: a region at a time, flooded from its first cell
  int regions = 0;
  uint32_t rem = pass;
  for (int guard = 0; guard < cells && __any(rem != 0); guard++) {
    const int r0 = __ffsll((unsigned long long)__ballot(rem != 0)) - 1;
    const uint32_t first = __shfl(rem, r0, 64);
    uint32_t cur = lane == r0 ? first & (0u - first) : 0u;
    for (int step = 0; step < cells; step++) {
      const uint32_t up = __shfl_up(cur, 1, 64), down = __shfl_down(cur, 1, 64);
      const uint32_t nx = (cur | (cur << 1) | (cur >> 1) | (lane > 0 ? up : 0u) | (lane < 63 ? down : 0u)) & rem;
      const bool grew = nx != cur;
      cur = nx;
      if (!__any(grew)) break;
    }
    rem &= ~cur;
    regions++;
  }
  stats[6] = regions;
  stats[7] = 0;
  stats[8] = 0;
  stats[9] = W * H;
  stats[10] = 0;
  __syncthreads();

  int status = -1, its[4] = {0, 0, 0, 0};
  int fx = 0, fy = 0, fair = 0, flost = 0, fkey = 0, fdepth = 0;
  const bool play = stats[0] == 1 && stats[2] == 1 && stats[4] == 1 && regions == 1;  // ddave_prob.py:164-165
  if (play && stats[3] > DD_MAX_DIAMONDS) {
    status = 5;
  } else if (play) {
    uint8_t *slot = a.ws + (size_t)lvl * a.ws_stride;
    uint4 *nodes = (uint4 *)slot;
    uint64_t *lefts = (uint64_t *)(slot + dd_nodes_per_stage(a.power) * 16);
    uint32_t *tags = (uint32_t *)(lefts + a.hash_cap);
    uint32_t *heap = tags + a.hash_cap;
    DdGame g;
    g.py = at_player / W + 1, g.px = at_player % W + 1;
    g.ky = at_key / W + 1, g.kx = at_key % W + 1;
    g.dy = at_exit / W + 1, g.dx = at_exit % W + 1;
    g.wh = W + 2 + H + 2;
    g.nd = stats[3];
    uint32_t fin = 0;
    int won = 0;
    status = 0;
    for (int stage = 0; stage < 4; stage++) {
      for (int i = lane; i < a.hash_cap / 4; i += 64) ((uint4 *)tags)[i] = make_uint4(0, 0, 0, 0);
      __syncthreads();
      int it = 0;
      if (lane == 0) {
        bool w;
        fin = dd_search(L, g, nodes, heap, tags, lefts, (uint32_t)a.hash_cap - 1u, a.power, 2 - stage, it, w);
        won = w ? 1 : 0;
      }
      its[stage] = __shfl(it, 0, 64);
      won = __shfl(won, 0, 64);
      __syncthreads();
      if (won) {
        status = stage + 1;
        break;
      }
    }
    // the returned node (solState) and its chain of actions, by lane 0
    int fj = 0, fh = 0, fcol = 0;
    if (lane == 0) {
      uint4 nd = nodes[fin];
      fx = dd_nx(nd), fy = dd_ny(nd), fair = dd_nair(nd), flost = dd_nlost(nd), fkey = dd_nkey(nd), fdepth = dd_ndepth(nd);
      fj = dd_njumps(nd);
      fcol = g.nd - __popcll(dd_nleft(nd));
      fh = dd_heuristic(g, fx, fy, fkey, dd_nleft(nd));
      if (a.moves && a.cap > 0) {
        int8_t *mv = a.moves + (size_t)lvl * a.cap;
        for (int p = fdepth - 1; p >= 0; p--) {  // depth <= power
          if (p < a.cap) mv[p] = (int8_t)dd_naction(nd);
          nd = nodes[dd_nparent(nd)];
        }
      }
    }
    fx = __shfl(fx, 0, 64), fy = __shfl(fy, 0, 64), fair = __shfl(fair, 0, 64), flost = __shfl(flost, 0, 64);
    fkey = __shfl(fkey, 0, 64), fdepth = __shfl(fdepth, 0, 64);
    stats[7] = __shfl(fj, 0, 64);
    stats[8] = __shfl(fcol, 0, 64);
    stats[9] = won ? 0 : __shfl(fh, 0, 64);
    stats[10] = won ? fdepth : 0;
  }
  if (a.moves && a.cap > 0) {
    int8_t *mv = a.moves + (size_t)lvl * a.cap;
    for (int p = fdepth + lane; p < a.cap; p += 64) mv[p] = -1;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < DD_STATS; k++) a.stats[(size_t)lvl * DD_STATS + k] = stats[k];
    if (a.length) a.length[lvl] = fdepth;
    if (a.play) {
      int32_t *p = a.play + (size_t)lvl * DD_PLAY;
      p[0] = status, p[1] = its[0], p[2] = its[1], p[3] = its[2], p[4] = its[3];
      p[5] = fx, p[6] = fy, p[7] = fair, p[8] = status >= 0 && status <= 4 ? 1 - flost : 0, p[9] = fkey, p[10] = stats[3];
      p[11] = fdepth;
    }
    if (a.error) a.error[lvl] = err;
  }
}

// dd_measures_kernel: one wave per map; the per-map body is meas_wave_map<7, 3, 512> of measures/pcgrl_measures_wave.h (ids
// masked to 3 bits; 7 is no counted tile).  The pairwise step is measures/pcgrl_measures.h's, launched as it is.
__global__ __launch_bounds__(64) void dd_measures_kernel(const MeasWaveArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t cells[DD_MAX_CELLS + 32];
  const int e = blockIdx.x;
  if (e >= a.n) return;
  meas_wave_map<DD_MEAS_TILES, DD_MEAS_PLANES, DD_MAX_CELLS>(a, e, cells);
}

#endif  // PCGRL_DD_KERNEL

}  // namespace pcgrl
