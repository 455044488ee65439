// mdungeon/pcgrl_mdungeon.h -- MiniDungeon levels on the device (include/pcgrl_amd_mdungeon.h): what MDungeonProblem.get_stats
// computes for an H x W map of 8 tile types (envs/probs/mdungeon/mdungeon_prob.py:151-171) -- six map statistics and the
// four-stage play-through of mdungeon/engine.py.  DESIGN.md section 32 has the rules with every quirk; tests/mdungeon_rules.py is
// the same in plain Python.  The layout is that of ddave/pcgrl_ddave.h (section 31); the level image, the node, the key and the
// transition are this game's.
//
// mdungeon_kernel: one 64-lane wave per level.
//   map       the level's bytes are staged in LDS with byte loads (any alignment; an id above 7 becomes solid and raises error
//             bit 0).
//   scans     lane-parallel: a lane counts the tiles of cells lane, lane + 64, ...; wave reductions.  Lane r < H then builds row
//             r's masks (solid, potion, treasure, goblin, ogre) and its items' row-major ordinals; the regions are peeled off one
//             at a time, a row per lane, the flood's neighbour rows taken by shuffles (every loop bounded by the cell count).
//   level     in LDS, with the solid border: solid[y] bit rows (y < H + 2 <= 18, x < W + 2 <= 34), ord[y][x] the item ordinal of
//             a cell (255: none).  Which ordinals are potions, treasures, goblins and ogres: four 64-bit masks, OR-reduced over
//             the wave into registers, with the player's and the door's positions.  A node's counters are popcounts of
//             consumed & type mask: the node carries none.
//   search    lane 0 alone, as smb_search (smb/pcgrl_smb.h has the reasons).  The A* open list is CPython's heapq
//             (md_heap_push / md_heap_pop: this unit's copy of dd_heap_push / dd_heap_pop, which sit under the Dave unit's
//             private macro), ordered with `<` alone by f = 2 * heuristic + (2 * balance) * depth + MD_F_BIAS, an exact integer
//             image of heuristic + balance * depth that is never negative.  The BFS pops in push order, which is the order of
//             the node array: its open list is an index into it.
//   memory    per level a workspace slot in HBM: nodes (16 B: x 6 | y 5 | health 3 | lost 1 | action 2 ; parent 16 | depth 14 ;
//             the 64-bit set of items still on the map), 4 * power + 1 of them -- an expansion pushes four and there are at most
//             `power` expansions -- reused by the next stage; the heap (4 B: f 16 | node 16), as many; the visited set,
//             open-addressed with linear probing over C >= 2 * power slots (a 32-bit tag: x, y, health and an occupied bit; the
//             64-bit item set beside it), whose tags the whole wave clears before each stage.  At most `power` keys are inserted,
//             so a probe meets a free slot within C steps.  Nodes and heap are written before they are read, so a dirty
//             workspace does not matter.
//   outputs   the returned node's parent chain gives the moves (lane 0); all lanes fill the tail with -1.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../measures/pcgrl_measures_wave.h"  // MeasWaveArgs, meas_wave_map

namespace pcgrl {

constexpr int MD_TILES = 8;
constexpr int MD_STATS = 11;  // player, exit, potions, treasures, enemies, regions, col-potions, col-treasures, col-enemies, dist-win, sol-length
constexpr int MD_PLAY = 12;
constexpr int MD_MAX_H = 16, MD_MAX_W = 32;
constexpr int MD_MAX_CELLS = MD_MAX_H * MD_MAX_W;  // 512
constexpr int MD_MAX_POWER = 16000;  // depth < 2^14; 4 * power + 1 nodes < 2^16
constexpr int MD_MAX_ITEMS = 64;     // the remaining potions, treasures and enemies are one 64-bit word
constexpr int MD_MAX_HEALTH = 5;
constexpr int MD_LW = MD_MAX_W + 2, MD_LH = MD_MAX_H + 2;
// heuristic = distance + 4 * (5 - health) - 4 * treasures >= -4 * 64, so 2 * heuristic + MD_F_BIAS >= 0; and
// 2 * heuristic + 2 * depth + bias <= 2 * (33 + 17 + 20) + 32 000 + 512 < 2^16
constexpr int MD_F_BIAS = 2 * 4 * MD_MAX_ITEMS;
constexpr int MD_MEAS_TILES = 8, MD_MEAS_PLANES = 3;

struct MdArgs {
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

__host__ __device__ inline int64_t md_nodes_per_stage(int power) { return 4 * (int64_t)power + 1; }
inline int32_t md_hash_cap(int power) {
  int32_t c = 16;
  while (c < 2 * power) c <<= 1;
  return c;
}
__host__ __device__ inline int64_t md_heap_bytes(int power) { return (md_nodes_per_stage(power) * 4 + 15) / 16 * 16; }
// one level's workspace slot: the nodes, the visited set's item words, its tags, the heap; a multiple of 16 bytes
inline int64_t md_ws_stride(int power) {
  return md_nodes_per_stage(power) * 16 + (int64_t)md_hash_cap(power) * 12 + md_heap_bytes(power);
}

hipError_t launch_mdungeon(const MdArgs &a, hipStream_t s);
hipError_t launch_md_measures(const MeasWaveArgs &a, hipStream_t s);

#ifdef PCGRL_MD_KERNEL  // (mdungeon/pcgrl_k_mdungeon.hip has it)

struct MdLds {
  uint8_t map[MD_MAX_CELLS];
  uint64_t solid[MD_LH];
  uint8_t ord[MD_LH * MD_LW];
};

// what the search reads besides the LDS level (lane 0's registers)
struct MdGame {
  int px, py, dx, dy;  // bordered coordinates
  int ni;              // items in the level, <= 64
  uint64_t potion, treasure, goblin, ogre;  // the ordinals of each item type
};

__device__ __forceinline__ int md_wave_sum(int v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int md_wave_max(int v) {
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ uint64_t md_wave_or(uint64_t v) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  for (int o = 32; o >= 1; o >>= 1) {
    lo |= (uint32_t)__shfl_xor((int)lo, o, 64);
    hi |= (uint32_t)__shfl_xor((int)hi, o, 64);
  }
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

__device__ __forceinline__ uint32_t md_key(uint32_t e) { return e >> 16; }

// heapq.heappush: the item goes to the end, then _siftdown(heap, 0, n - 1)
__device__ __forceinline__ void md_heap_push(uint32_t *heap, int &n, uint32_t item) {
  int pos = n++;
  while (pos > 0) {
    const int pp = (pos - 1) >> 1;
    const uint32_t parent = heap[pp];
    if (!(md_key(item) < md_key(parent))) break;
    heap[pos] = parent;
    pos = pp;
  }
  heap[pos] = item;
}

// heapq.heappop: the last item replaces the root, _siftup(heap, 0)
__device__ __forceinline__ uint32_t md_heap_pop(uint32_t *heap, int &n) {
  const uint32_t last = heap[--n];
  if (n == 0) return last;
  const uint32_t ret = heap[0];
  int pos = 0, child = 1;
  while (child < n) {  // bubble the smaller child up until a leaf
    uint32_t c = heap[child];
    if (child + 1 < n) {
      const uint32_t r = heap[child + 1];
      if (!(md_key(c) < md_key(r))) {
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
    if (!(md_key(last) < md_key(parent))) break;
    heap[pos] = parent;
    pos = pp;
  }
  heap[pos] = last;
  return ret;
}

__device__ __forceinline__ uint4 md_pack(int x, int y, int health, int action, uint32_t parent, int depth, uint64_t left) {
  return make_uint4((uint32_t)x | ((uint32_t)y << 6) | ((uint32_t)health << 11) | ((uint32_t)(health <= 0) << 14) |
                        ((uint32_t)action << 15),
                    parent | ((uint32_t)depth << 16), (uint32_t)left, (uint32_t)(left >> 32));
}
__device__ __forceinline__ int md_nx(uint4 v) { return v.x & 0x3F; }
__device__ __forceinline__ int md_ny(uint4 v) { return (v.x >> 6) & 0x1F; }
__device__ __forceinline__ int md_nhealth(uint4 v) { return (v.x >> 11) & 7; }
__device__ __forceinline__ int md_nlost(uint4 v) { return (v.x >> 14) & 1; }
__device__ __forceinline__ int md_naction(uint4 v) { return (v.x >> 15) & 3; }
__device__ __forceinline__ uint32_t md_nparent(uint4 v) { return v.y & 0xFFFFu; }
__device__ __forceinline__ int md_ndepth(uint4 v) { return (v.y >> 16) & 0x3FFF; }
__device__ __forceinline__ uint64_t md_nleft(uint4 v) { return (uint64_t)v.z | ((uint64_t)v.w << 32); }

// State.getHeuristic (engine.py:285-289); the collected treasures are those of the level that are no longer on the map
__device__ __forceinline__ int md_heuristic(const MdGame &g, int x, int y, int health, uint64_t left) {
  return abs(x - g.dx) + abs(y - g.dy) + 4 * (MD_MAX_HEALTH - health) - 4 * __popcll(g.treasure & ~left);
}

__device__ __forceinline__ bool md_solid(const MdLds &L, int x, int y) { return (L.solid[y] >> x) & 1u; }

// The visited set: true when (tag, left) is in it, else it goes in.  At most `power` <= C / 2 keys are ever inserted, so the
// probe ends at a free slot; the bound is for the compiler's and the reader's peace.
__device__ __forceinline__ bool md_visited(uint32_t *tags, uint64_t *lefts, uint32_t capmask, uint32_t tag, uint64_t left) {
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
__device__ inline uint32_t md_search(const MdLds &L, const MdGame &g, uint4 *nodes, uint32_t *heap, uint32_t *tags, uint64_t *lefts,
                                     uint32_t capmask, int power, int balance2, int &iterations, bool &won) {
  const bool astar = balance2 >= 0;
  const uint64_t all = g.ni >= 64 ? ~0ull : (1ull << g.ni) - 1ull;
  nodes[0] = md_pack(g.px, g.py, MD_MAX_HEALTH, 0, 0, 0, all);
  int nn = 1, hn = 0, head = 0, it = 0;
  if (astar) {
    heap[0] = (uint32_t)(2 * md_heuristic(g, g.px, g.py, MD_MAX_HEALTH, all) + MD_F_BIAS) << 16;
    hn = 1;
  }
  uint32_t best = 0;
  int best_h = 0x7FFFFFFF, best_depth = 0;
  won = false;
  while (it < power && (astar ? hn > 0 : head < nn)) {
    it++;
    const uint32_t cur = astar ? (md_heap_pop(heap, hn) & 0xFFFFu) : (uint32_t)head++;
    const uint4 nd = nodes[cur];
    if (md_nlost(nd)) continue;
    const int x = md_nx(nd), y = md_ny(nd), health = md_nhealth(nd), depth = md_ndepth(nd);
    const uint64_t left = md_nleft(nd);
    if (x == g.dx && y == g.dy) {
      best = cur;
      won = true;
      break;
    }
    if (md_visited(tags, lefts, capmask, 0x80000000u | (uint32_t)x | ((uint32_t)y << 6) | ((uint32_t)health << 11), left)) continue;
    const int h = md_heuristic(g, x, y, health, left);
    if (h < best_h || (h == best_h && depth < best_depth)) {
      best = cur;
      best_h = h;
      best_depth = depth;
    }
    // State.update (engine.py:254-270) for directions 0..3 = left, right, up, down
    for (int a = 0; a < 4; a++) {
      const int tx = x + (a == 0 ? -1 : a == 1 ? 1 : 0), ty = y + (a == 2 ? -1 : a == 3 ? 1 : 0);
      int cx = x, cy = y, ch = health;
      uint64_t cleft = left;
      if (!md_solid(L, tx, ty)) {
        cx = tx, cy = ty;
        // updatePlayer (engine.py:229-252): a cell holds one item, so the order of its three tests does not show
        const uint32_t o = L.ord[cy * MD_LW + cx];
        if (o < 64 && ((cleft >> o) & 1ull)) {
          const uint64_t bit = 1ull << o;
          cleft &= ~bit;
          if (g.potion & bit) ch = min(ch + 2, MD_MAX_HEALTH);
          else if (g.goblin & bit) ch = max(ch - 1, 0);
          else if (g.ogre & bit) ch = max(ch - 2, 0);
        }
      }
      nodes[nn] = md_pack(cx, cy, ch, a, cur, depth + 1, cleft);
      if (astar) {
        const int f = 2 * md_heuristic(g, cx, cy, ch, cleft) + balance2 * (depth + 1) + MD_F_BIAS;
        md_heap_push(heap, hn, ((uint32_t)f << 16) | (uint32_t)nn);
      }
      nn++;
    }
  }
  iterations = it;
  return best;
}

__global__ __launch_bounds__(64) void mdungeon_kernel(const MdArgs a) {
  __shared__ MdLds L;
  const int lvl = blockIdx.x, lane = threadIdx.x;
  if (lvl >= a.n) return;
  const int H = a.h, W = a.w, cells = H * W;
  const uint8_t *grid = a.grids + (size_t)lvl * cells;
  bool bad = false;
  for (int i = lane; i < cells; i += 64) {
    uint8_t t = grid[i];
    if (t >= MD_TILES) {
      bad = true;
      t = 1;
    }
    L.map[i] = t;
  }
  const uint32_t err = __any(bad) ? 1u : 0u;
  __syncthreads();

  // the counts, and where the player and the door are (the last of each; the game needs exactly one)
  int cnt_player = 0, cnt_exit = 0, cnt_potion = 0, cnt_treasure = 0, cnt_enemy = 0;
  int at_player = -1, at_exit = -1;
  for (int i = lane; i < cells; i += 64) {
    const int t = L.map[i];
    cnt_potion += t == 4;
    cnt_treasure += t == 5;
    cnt_enemy += t == 6 || t == 7;
    if (t == 2) {
      cnt_player++;
      at_player = i;
    }
    if (t == 3) {
      cnt_exit++;
      at_exit = i;
    }
  }
  int32_t stats[MD_STATS];
  stats[0] = md_wave_sum(cnt_player);
  stats[1] = md_wave_sum(cnt_exit);
  stats[2] = md_wave_sum(cnt_potion);
  stats[3] = md_wave_sum(cnt_treasure);
  stats[4] = md_wave_sum(cnt_enemy);
  at_player = md_wave_max(at_player);
  at_exit = md_wave_max(at_exit);
  const int items = stats[2] + stats[3] + stats[4];

  // lane r < H: row r's masks, its items' ordinals, and its rows of the bordered level
  uint32_t pass = 0, solid = 0, pot = 0, tre = 0, gob = 0, ogr = 0;
  if (lane < H)
    for (int c = 0; c < W; c++) {
      const int t = L.map[lane * W + c];
      solid |= (uint32_t)(t == 1) << c;
      pot |= (uint32_t)(t == 4) << c;
      tre |= (uint32_t)(t == 5) << c;
      gob |= (uint32_t)(t == 6) << c;
      ogr |= (uint32_t)(t == 7) << c;
    }
  if (lane < H) pass = ~solid & (W == 32 ? ~0u : (1u << W) - 1u);
  const uint32_t item = pot | tre | gob | ogr;
  const int row_items = __popc(item);
  int before = 0;  // items in the rows above
  for (int r = 0; r < MD_MAX_H - 1; r++) {
    const int v = __shfl(row_items, r, 64);
    if (r < lane) before += v;
  }
  uint64_t m_pot = 0, m_tre = 0, m_gob = 0, m_ogr = 0;
  if (lane < H) {
    L.solid[lane + 1] = ((uint64_t)solid << 1) | 1ull | (1ull << (W + 1));
    for (int c = 0; c < W; c++) {
      const int o = before + __popc(item & ((1u << c) - 1u));
      const bool is = (item >> c) & 1u;
      L.ord[(lane + 1) * MD_LW + c + 1] = is ? (uint8_t)min(o, 255) : (uint8_t)255;
      if (is && o < 64) {  // past 64 the level is not searched
        const uint64_t bit = 1ull << o;
        if ((pot >> c) & 1u) m_pot |= bit;
        if ((tre >> c) & 1u) m_tre |= bit;
        if ((gob >> c) & 1u) m_gob |= bit;
        if ((ogr >> c) & 1u) m_ogr |= bit;
      }
    }
  } else if (lane < H + 2) {
    const int y = lane == H ? 0 : H + 1;
    L.solid[y] = (1ull << (W + 2)) - 1ull;
  }
  m_pot = md_wave_or(m_pot);
  m_tre = md_wave_or(m_tre);
  m_gob = md_wave_or(m_gob);
  m_ogr = md_wave_or(m_ogr);

  // calc_num_regions (helper.py:200-210) over everything but solid: a region at a time, flooded from its first cell
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
  stats[5] = regions;
  stats[6] = 0;
  stats[7] = 0;
  stats[8] = 0;
  stats[9] = W * H;
  stats[10] = 0;
  __syncthreads();

  int status = -1, its[4] = {0, 0, 0, 0};
  int fx = 0, fy = 0, fhealth = 0, fdepth = 0;
  const bool play = stats[0] == 1 && stats[1] == 1 && regions == 1;  // mdungeon_prob.py:166
  if (play && items > MD_MAX_ITEMS) {
    status = 5;
  } else if (play) {
    uint8_t *slot = a.ws + (size_t)lvl * a.ws_stride;
    uint4 *nodes = (uint4 *)slot;
    uint64_t *lefts = (uint64_t *)(slot + md_nodes_per_stage(a.power) * 16);
    uint32_t *tags = (uint32_t *)(lefts + a.hash_cap);
    uint32_t *heap = tags + a.hash_cap;
    MdGame g;
    g.py = at_player / W + 1, g.px = at_player % W + 1;
    g.dy = at_exit / W + 1, g.dx = at_exit % W + 1;
    g.ni = items;
    g.potion = m_pot, g.treasure = m_tre, g.goblin = m_gob, g.ogre = m_ogr;
    uint32_t fin = 0;
    int won = 0;
    status = 0;
    for (int stage = 0; stage < 4; stage++) {
      for (int i = lane; i < a.hash_cap / 4; i += 64) ((uint4 *)tags)[i] = make_uint4(0, 0, 0, 0);
      __syncthreads();
      int it = 0;
      if (lane == 0) {
        bool w;
        fin = md_search(L, g, nodes, heap, tags, lefts, (uint32_t)a.hash_cap - 1u, a.power, 2 - stage, it, w);
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
    int fh = 0, fpot = 0, ftre = 0, fene = 0;
    if (lane == 0) {
      uint4 nd = nodes[fin];
      fx = md_nx(nd), fy = md_ny(nd), fhealth = md_nhealth(nd), fdepth = md_ndepth(nd);
      const uint64_t gone = ~md_nleft(nd);
      fpot = __popcll(g.potion & gone);
      ftre = __popcll(g.treasure & gone);
      fene = __popcll((g.goblin | g.ogre) & gone);
      fh = md_heuristic(g, fx, fy, fhealth, md_nleft(nd));
      if (a.moves && a.cap > 0) {
        int8_t *mv = a.moves + (size_t)lvl * a.cap;
        for (int p = fdepth - 1; p >= 0; p--) {  // depth <= power
          if (p < a.cap) mv[p] = (int8_t)md_naction(nd);
          nd = nodes[md_nparent(nd)];
        }
      }
    }
    fx = __shfl(fx, 0, 64), fy = __shfl(fy, 0, 64), fhealth = __shfl(fhealth, 0, 64), fdepth = __shfl(fdepth, 0, 64);
    stats[6] = __shfl(fpot, 0, 64);
    stats[7] = __shfl(ftre, 0, 64);
    stats[8] = __shfl(fene, 0, 64);
    stats[9] = won ? 0 : __shfl(fh, 0, 64);
    stats[10] = won ? fdepth : 0;
  }
  if (a.moves && a.cap > 0) {
    int8_t *mv = a.moves + (size_t)lvl * a.cap;
    for (int p = fdepth + lane; p < a.cap; p += 64) mv[p] = -1;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < MD_STATS; k++) a.stats[(size_t)lvl * MD_STATS + k] = stats[k];
    if (a.length) a.length[lvl] = fdepth;
    if (a.play) {
      int32_t *p = a.play + (size_t)lvl * MD_PLAY;
      p[0] = status, p[1] = its[0], p[2] = its[1], p[3] = its[2], p[4] = its[3];
      p[5] = fx, p[6] = fy, p[7] = fhealth, p[8] = stats[6], p[9] = stats[7], p[10] = stats[8];
      p[11] = fdepth;
    }
    if (a.error) a.error[lvl] = err;
  }
}

// md_measures_kernel: one wave per map; the per-map body is meas_wave_map<8, 3, 512> of measures/pcgrl_measures_wave.h (ids
// masked to 3 bits: every value is a counted tile).  The pairwise step is measures/pcgrl_measures.h's, launched as it is.
__global__ __launch_bounds__(64) void md_measures_kernel(const MeasWaveArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t cells[MD_MAX_CELLS + 32];
  const int e = blockIdx.x;
  if (e >= a.n) return;
  meas_wave_map<MD_MEAS_TILES, MD_MEAS_PLANES, MD_MAX_CELLS>(a, e, cells);
}

#endif  // PCGRL_MD_KERNEL

}  // namespace pcgrl
