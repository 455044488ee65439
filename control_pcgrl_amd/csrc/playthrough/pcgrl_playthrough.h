// playthrough/pcgrl_playthrough.h -- what the solver play-throughs of Dangerous Dave (ddave/pcgrl_ddave.h) and MiniDungeon
// (mdungeon/pcgrl_mdungeon.h) share, written once: the launch arguments and the workspace arithmetic (host), and under
// PCGRL_PT_KERNEL (or PCGRL_KERNEL_TU) the wave reductions, CPython's heapq, the visited set, the region count, the level's
// bordered rows, the search loop and the kernel body, the last two over a per-game policy.  smb/pcgrl_smb.h takes the heap and
// the wave sum from here.  DESIGN.md section 39.
//
// pt_level<G>: one 64-lane wave per level.
//   map       the level's bytes are staged in LDS with byte loads (any alignment; an id of G::TILES or above becomes solid and
//             raises error bit 0).
//   scans     G::scan, lane-parallel: the map's statistics by wave reductions, then lane r < H builds row r's masks and its
//             items' row-major ordinals (pt_level_rows); the regions are peeled off one at a time, a row per lane, the flood's
//             neighbour rows taken by shuffles (pt_regions; every loop bounded by the cell count).
//   level     in LDS, with the solid border: solid[y] bit rows (y < H + 2 <= 18, x < W + 2 <= 34), ord[y][x] the item ordinal
//             of a cell (255: none), and what else the game keeps; the positions in registers (G::Game).
//   search    lane 0 alone, as smb_search (smb/pcgrl_smb.h has the reasons): the cost of an iteration is the chain of dependent
//             loads of the heap's sifts and of the hash probe, hidden by occupancy.  The A* open list is CPython's heapq with a
//             16-bit node index, ordered with `<` alone by f = 2 * heuristic + (2 * balance) * depth + G::F_BIAS, an exact
//             integer image of heuristic + balance * depth that is never negative.  The BFS pops in push order, which is the
//             order of the node array: its open list is an index into it.
//   memory    per level a workspace slot in HBM: nodes (16 B: the state word x 6 | y 5 | game 3 | lost 1 | action 2 | game 15 ;
//             parent 16 | depth 14 ; the 64-bit set of items still on the map), 4 * power + 1 of them -- an expansion pushes
//             four and there are at most `power` expansions -- reused by the next stage; the heap (4 B: f 16 | node 16), as
//             many; the visited set, open-addressed with linear probing over C >= 2 * power slots (a 32-bit tag: x, y, the
//             game's bits and an occupied bit; the 64-bit item set beside it), whose tags the whole wave clears before each
//             stage.  At most `power` keys are inserted, so a probe meets a free slot within C steps.  Nodes and heap are
//             written before they are read, so a dirty workspace does not matter.
//   outputs   the returned node's parent chain gives the moves (lane 0); all lanes fill the tail with -1.
//
// The policy G (DdPolicy, MdPolicy) has the types Lds (with map, solid and ord), Game (with items), Scan and State (a node's
// state word in separate fields, x and y among them), the constants TILES, REGIONS (the statistics column of the region
// count) and F_BIAS, and the static functions
//   scan(L, H, W, stats, pc, s)        the map's statistics and play columns, the LDS level, s; returns the lane's row of
//                                      region cells
//   played(stats)                      whether get_stats plays the level, its one region apart
//   too_many(stats)                    more items than the 64-bit set holds: status 5, not searched
//   game(s, stats, H, W)               the search's registers
//   unpack(word), pack(state)          between a node's state word and State
//   root(g)                            the start's State
//   wins(g, state), tag(state), heuristic(g, state, left)
//   step(L, g, state, rows, left, a)   State.update for action a: the child's State, `left` updated in place
//   finish(g, node, stats, pc)         the game's statistics and play columns of the returned node
// Everything inlines into the game's kernel: no run-time choice of game anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcgrl {

constexpr int PT_STATS = 11, PT_PLAY = 12;  // both games: dist-win and sol-length are statistics 9 and 10
constexpr int PT_MAX_H = 16, PT_MAX_W = 32;
constexpr int PT_MAX_POWER = 16000;  // depth < 2^14; 4 * power + 1 nodes < 2^16
constexpr int PT_LW = PT_MAX_W + 2, PT_LH = PT_MAX_H + 2;

struct PtArgs {
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

__host__ __device__ inline int64_t pt_nodes_per_stage(int power) { return 4 * (int64_t)power + 1; }
inline int32_t pt_hash_cap(int power) {
  int32_t c = 16;
  while (c < 2 * power) c <<= 1;
  return c;
}
__host__ __device__ inline int64_t pt_heap_bytes(int power) { return (pt_nodes_per_stage(power) * 4 + 15) / 16 * 16; }
// one level's workspace slot: the nodes, the visited set's item words, its tags, the heap; a multiple of 16 bytes
inline int64_t pt_ws_stride(int power) {
  return pt_nodes_per_stage(power) * 16 + (int64_t)pt_hash_cap(power) * 12 + pt_heap_bytes(power);
}

#if defined(PCGRL_PT_KERNEL) || defined(PCGRL_KERNEL_TU)  // (the two games' kernel units; the smb kernel units)

__device__ __forceinline__ int pt_wave_sum(int v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int pt_wave_max(int v) {
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ uint64_t pt_wave_or(uint64_t v) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  for (int o = 32; o >= 1; o >>= 1) {
    lo |= (uint32_t)__shfl_xor((int)lo, o, 64);
    hi |= (uint32_t)__shfl_xor((int)hi, o, 64);
  }
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// CPython's heapq over 32-bit entries, f above SHIFT bits of node index, ordered by f alone with `<`: the sift order decides
// which of several equal-f nodes is expanded first.  heappush: the item goes to the end, then _siftdown(heap, 0, n - 1)
template <int SHIFT>
__device__ __forceinline__ void pt_heap_push(uint32_t *heap, int &n, uint32_t item) {
  int pos = n++;
  while (pos > 0) {
    const int pp = (pos - 1) >> 1;
    const uint32_t parent = heap[pp];
    if (!((item >> SHIFT) < (parent >> SHIFT))) break;
    heap[pos] = parent;
    pos = pp;
  }
  heap[pos] = item;
}

// heapq.heappop: the last item replaces the root, _siftup(heap, 0)
template <int SHIFT>
__device__ __forceinline__ uint32_t pt_heap_pop(uint32_t *heap, int &n) {
  const uint32_t last = heap[--n];
  if (n == 0) return last;
  const uint32_t ret = heap[0];
  int pos = 0, child = 1;
  while (child < n) {  // bubble the smaller child up until a leaf
    uint32_t c = heap[child];
    if (child + 1 < n) {
      const uint32_t r = heap[child + 1];
      if (!((c >> SHIFT) < (r >> SHIFT))) {
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
    if (!((last >> SHIFT) < (parent >> SHIFT))) break;
    heap[pos] = parent;
    pos = pp;
  }
  heap[pos] = last;
  return ret;
}

// A node: the state word (a game packs its own bits around x, y and lost, and leaves the action's free), its parent and depth,
// and the items still on the map.
__device__ __forceinline__ uint4 pt_node(uint32_t state, int action, uint32_t parent, int depth, uint64_t left) {
  return make_uint4(state | ((uint32_t)action << 15), parent | ((uint32_t)depth << 16), (uint32_t)left, (uint32_t)(left >> 32));
}
__device__ __forceinline__ int pt_sx(uint32_t state) { return state & 0x3F; }
__device__ __forceinline__ int pt_sy(uint32_t state) { return (state >> 6) & 0x1F; }
__device__ __forceinline__ int pt_slost(uint32_t state) { return (state >> 14) & 1; }
__device__ __forceinline__ int pt_naction(uint4 v) { return (v.x >> 15) & 3; }
__device__ __forceinline__ uint32_t pt_nparent(uint4 v) { return v.y & 0xFFFFu; }
__device__ __forceinline__ int pt_ndepth(uint4 v) { return (v.y >> 16) & 0x3FFF; }
__device__ __forceinline__ uint64_t pt_nleft(uint4 v) { return (uint64_t)v.z | ((uint64_t)v.w << 32); }

// The visited set: true when (tag, left) is in it, else it goes in.  At most `power` <= C / 2 keys are ever inserted, so the
// probe ends at a free slot; the bound is for the compiler's and the reader's peace.
__device__ __forceinline__ bool pt_visited(uint32_t *tags, uint64_t *lefts, uint32_t capmask, uint32_t tag, uint64_t left) {
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

// calc_num_regions (helper.py:200-210) over the cells in `pass` (lane r: row r's bits): a region at a time, flooded from its
// first cell
__device__ __forceinline__ int pt_regions(uint32_t pass, int cells) {
  const int lane = threadIdx.x;
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
  return regions;
}

// The bordered level's rows: lane r < H writes row r + 1 of `solid` from its row's solid bits and the row-major ordinals of its
// row's items into `ord` (255: no item, or one past the 255th); lanes H and H + 1 write the two border rows.  Returns the items
// in the rows above the lane's.
__device__ __forceinline__ int pt_level_rows(uint64_t *solid, uint8_t *ord, int H, int W, uint32_t row_solid, uint32_t row_item) {
  const int lane = threadIdx.x;
  const int row_items = __popc(row_item);
  int before = 0;
  for (int r = 0; r < PT_MAX_H - 1; r++) {
    const int v = __shfl(row_items, r, 64);
    if (r < lane) before += v;
  }
  if (lane < H) {
    solid[lane + 1] = ((uint64_t)row_solid << 1) | 1ull | (1ull << (W + 1));
    for (int c = 0; c < W; c++) {
      const int o = before + __popc(row_item & ((1u << c) - 1u));
      ord[(lane + 1) * PT_LW + c + 1] = ((row_item >> c) & 1u) ? (uint8_t)min(o, 255) : (uint8_t)255;
    }
  } else if (lane < H + 2) {
    solid[lane == H ? 0 : H + 1] = (1ull << (W + 2)) - 1ull;
  }
  return before;
}

// The solid rows around a node, y - 1, y and y + 1 (a node is never on a border row): read once per node, before its four
// children, which all test these three.
struct PtRows {
  uint64_t above, here, below;
};
__device__ __forceinline__ bool pt_solid(uint64_t row, int x) { return (row >> x) & 1u; }

// One of the four searches (one lane): AStarAgent.getSolution with balance2 / 2 (engine.py:105-129), or BFSAgent.getSolution
// when balance2 < 0 (engine.py:61-81).  Returns the node it ends on -- the winner, else the best node -- and the iterations it
// ran.  The tags must be zero on entry.
template <class G>
__device__ inline uint32_t pt_search(const typename G::Lds &L, const typename G::Game &g, uint4 *nodes, uint32_t *heap,
                                     uint32_t *tags, uint64_t *lefts, uint32_t capmask, int power, int balance2, int &iterations,
                                     bool &won) {
  const bool astar = balance2 >= 0;
  const uint64_t all = g.items >= 64 ? ~0ull : (1ull << g.items) - 1ull;
  nodes[0] = pt_node(G::pack(G::root(g)), 0, 0, 0, all);
  int nn = 1, hn = 0, head = 0, it = 0;
  if (astar) {
    heap[0] = (uint32_t)(2 * G::heuristic(g, G::root(g), all) + G::F_BIAS) << 16;
    hn = 1;
  }
  uint32_t best = 0;
  int best_h = 0x7FFFFFFF, best_depth = 0;
  won = false;
  while (it < power && (astar ? hn > 0 : head < nn)) {
    it++;
    const uint32_t cur = astar ? (pt_heap_pop<16>(heap, hn) & 0xFFFFu) : (uint32_t)head++;
    const uint4 nd = nodes[cur];
    if (pt_slost(nd.x)) continue;
    const typename G::State s = G::unpack(nd.x);
    const int depth = pt_ndepth(nd);
    const uint64_t left = pt_nleft(nd);
    if (G::wins(g, s)) {
      best = cur;
      won = true;
      break;
    }
    if (pt_visited(tags, lefts, capmask, G::tag(s), left)) continue;
    const int h = G::heuristic(g, s, left);
    if (h < best_h || (h == best_h && depth < best_depth)) {
      best = cur;
      best_h = h;
      best_depth = depth;
    }
    const PtRows rows = {L.solid[s.y - 1], L.solid[s.y], L.solid[s.y + 1]};
    for (int a = 0; a < 4; a++) {
      uint64_t cleft = left;
      const typename G::State child = G::step(L, g, s, rows, cleft, a);
      nodes[nn] = pt_node(G::pack(child), a, cur, depth + 1, cleft);
      if (astar) {
        const int f = 2 * G::heuristic(g, child, cleft) + balance2 * (depth + 1) + G::F_BIAS;
        pt_heap_push<16>(heap, hn, ((uint32_t)f << 16) | (uint32_t)nn);
      }
      nn++;
    }
  }
  iterations = it;
  return best;
}

// The body of a game's kernel: block `blockIdx.x`, one wave, evaluates level `blockIdx.x`.
template <class G>
__device__ __forceinline__ void pt_level(const PtArgs &a, typename G::Lds &L) {
  const int lvl = blockIdx.x, lane = threadIdx.x;
  if (lvl >= a.n) return;
  const int H = a.h, W = a.w, cells = H * W;
  const uint8_t *grid = a.grids + (size_t)lvl * cells;
  bool bad = false;
  for (int i = lane; i < cells; i += 64) {
    uint8_t t = grid[i];
    if (t >= G::TILES) {
      bad = true;
      t = 1;
    }
    L.map[i] = t;
  }
  const uint32_t err = __any(bad) ? 1u : 0u;
  __syncthreads();

  int32_t stats[PT_STATS] = {}, pc[6] = {};  // pc: the play columns 5..10
  typename G::Scan sc;
  const int regions = pt_regions(G::scan(L, H, W, stats, pc, sc), cells);
  stats[G::REGIONS] = regions;
  stats[9] = W * H;
  __syncthreads();

  int status = -1, its[4] = {0, 0, 0, 0}, fdepth = 0;
  const bool play = G::played(stats) && regions == 1;
  if (play && G::too_many(stats)) {
    status = 5;
  } else if (play) {
    uint8_t *slot = a.ws + (size_t)lvl * a.ws_stride;
    uint4 *nodes = (uint4 *)slot;
    uint64_t *lefts = (uint64_t *)(slot + pt_nodes_per_stage(a.power) * 16);
    uint32_t *tags = (uint32_t *)(lefts + a.hash_cap);
    uint32_t *heap = tags + a.hash_cap;
    const typename G::Game g = G::game(sc, stats, H, W);
    uint32_t fin = 0;
    int won = 0;
    status = 0;
    for (int stage = 0; stage < 4; stage++) {
      for (int i = lane; i < a.hash_cap / 4; i += 64) ((uint4 *)tags)[i] = make_uint4(0, 0, 0, 0);
      __syncthreads();
      int it = 0;
      if (lane == 0) {
        bool w;
        fin = pt_search<G>(L, g, nodes, heap, tags, lefts, (uint32_t)a.hash_cap - 1u, a.power, 2 - stage, it, w);
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
    if (lane == 0) {
      uint4 nd = nodes[fin];
      fdepth = pt_ndepth(nd);
      pc[0] = pt_sx(nd.x), pc[1] = pt_sy(nd.x);
      G::finish(g, nd, stats, pc);
      stats[9] = won ? 0 : G::heuristic(g, G::unpack(nd.x), pt_nleft(nd));
      stats[10] = won ? fdepth : 0;
      if (a.moves && a.cap > 0) {
        int8_t *mv = a.moves + (size_t)lvl * a.cap;
        for (int p = fdepth - 1; p >= 0; p--) {  // depth <= power
          if (p < a.cap) mv[p] = (int8_t)pt_naction(nd);
          nd = nodes[pt_nparent(nd)];
        }
      }
    }
    fdepth = __shfl(fdepth, 0, 64);
  }
  if (a.moves && a.cap > 0) {
    int8_t *mv = a.moves + (size_t)lvl * a.cap;
    for (int p = fdepth + lane; p < a.cap; p += 64) mv[p] = -1;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < PT_STATS; k++) a.stats[(size_t)lvl * PT_STATS + k] = stats[k];
    if (a.length) a.length[lvl] = fdepth;
    if (a.play) {
      int32_t *p = a.play + (size_t)lvl * PT_PLAY;
      p[0] = status, p[1] = its[0], p[2] = its[1], p[3] = its[2], p[4] = its[3];
#pragma unroll
      for (int k = 0; k < 6; k++) p[5 + k] = pc[k];
      p[11] = fdepth;
    }
    if (a.error) a.error[lvl] = err;
  }
}

#endif  // PCGRL_PT_KERNEL || PCGRL_KERNEL_TU

}  // namespace pcgrl
