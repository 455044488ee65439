// mdungeon/pcgrl_mdungeon.h -- MiniDungeon levels on the device (include/pcgrl_amd_mdungeon.h): what MDungeonProblem.get_stats
// computes for an H x W map of 8 tile types (envs/probs/mdungeon/mdungeon_prob.py:151-171) -- six map statistics and the
// four-stage play-through of mdungeon/engine.py.  DESIGN.md section 32 has the rules with every quirk; tests/mdungeon_rules.py is
// the same in plain Python.
//
// mdungeon_kernel: one 64-lane wave per level, pt_level<MdPolicy> of playthrough/pcgrl_playthrough.h.  That header has the
// kernel's layout, the search loop, the open list, the visited set, the region count and the workspace; this one has what is
// MiniDungeon's:
//   scans     a lane counts the tiles of cells lane, lane + 64, ...; lane r < H builds row r's masks (solid, potion, treasure,
//             goblin, ogre).  The regions are everything but solid.
//   level     the shared solid[y] and ord[y][x] (the items' ordinals) alone.  Which ordinals are potions, treasures, goblins and
//             ogres: four 64-bit masks, OR-reduced over the wave into registers, with the player's and the door's positions.  A
//             node's counters are popcounts of consumed & type mask: the node carries none.
//   node      MdState: the state word's own bits are health 3 (bits 11-13); lost is health 0.  The visited tag is x, y, health
//             and an occupied bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../measures/pcgrl_measures_wave.h"  // MeasWaveArgs, meas_wave_map
#include "../playthrough/pcgrl_playthrough.h"  // PtArgs, the workspace, pt_level

namespace pcgrl {

constexpr int MD_TILES = 8;
constexpr int MD_STATS = PT_STATS;  // player, exit, potions, treasures, enemies, regions, col-potions, col-treasures, col-enemies, dist-win, sol-length
constexpr int MD_MAX_H = PT_MAX_H, MD_MAX_W = PT_MAX_W;
constexpr int MD_MAX_CELLS = MD_MAX_H * MD_MAX_W;  // 512
constexpr int MD_MAX_ITEMS = 64;  // the remaining potions, treasures and enemies are a node's one 64-bit word
constexpr int MD_MAX_HEALTH = 5;
// heuristic = distance + 4 * (5 - health) - 4 * treasures >= -4 * 64, so 2 * heuristic + MD_F_BIAS >= 0; and
// 2 * heuristic + 2 * depth + bias <= 2 * (33 + 17 + 20) + 32 000 + 512 < 2^16
constexpr int MD_F_BIAS = 2 * 4 * MD_MAX_ITEMS;
constexpr int MD_MEAS_TILES = 8, MD_MEAS_PLANES = 3;

hipError_t launch_mdungeon(const PtArgs &a, hipStream_t s);
hipError_t launch_md_measures(const MeasWaveArgs &a, hipStream_t s);

#ifdef PCGRL_MD_KERNEL  // (mdungeon/pcgrl_k_mdungeon.hip has it, with PCGRL_PT_KERNEL)

struct MdLds {
  uint8_t map[MD_MAX_CELLS];
  uint64_t solid[PT_LH];
  uint8_t ord[PT_LH * PT_LW];
};

// what the search reads besides the LDS level (lane 0's registers)
struct MdGame {
  int px, py, dx, dy;  // bordered coordinates
  int items;           // items in the level, <= 64
  uint64_t potion, treasure, goblin, ogre;  // the ordinals of each item type
};

// where the player and the door are (the last cell of each; the game needs exactly one), and the ordinals of each item type
struct MdScan {
  int at_player, at_exit;
  uint64_t potion, treasure, goblin, ogre;
};

struct MdState {
  int x, y, health;
};

struct MdPolicy {
  using Lds = MdLds;
  using Game = MdGame;
  using Scan = MdScan;
  using State = MdState;
  static constexpr int TILES = MD_TILES, REGIONS = 5, F_BIAS = MD_F_BIAS;

  static __device__ __forceinline__ uint32_t scan(MdLds &L, int H, int W, int32_t *stats, int32_t *pc, MdScan &s) {
    const int lane = threadIdx.x, cells = H * W;
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
    stats[0] = pt_wave_sum(cnt_player);
    stats[1] = pt_wave_sum(cnt_exit);
    stats[2] = pt_wave_sum(cnt_potion);
    stats[3] = pt_wave_sum(cnt_treasure);
    stats[4] = pt_wave_sum(cnt_enemy);
    s.at_player = pt_wave_max(at_player);
    s.at_exit = pt_wave_max(at_exit);

    // lane r < H: row r's masks, its rows of the bordered level, and the type of each of its items' ordinals
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
    const int before = pt_level_rows(L.solid, L.ord, H, W, solid, item);
    uint64_t m_pot = 0, m_tre = 0, m_gob = 0, m_ogr = 0;
    for (int c = 0; c < W; c++) {
      const int o = before + __popc(item & ((1u << c) - 1u));
      if (((item >> c) & 1u) && o < 64) {  // past 64 the level is not searched
        const uint64_t bit = 1ull << o;
        if ((pot >> c) & 1u) m_pot |= bit;
        if ((tre >> c) & 1u) m_tre |= bit;
        if ((gob >> c) & 1u) m_gob |= bit;
        if ((ogr >> c) & 1u) m_ogr |= bit;
      }
    }
    s.potion = pt_wave_or(m_pot);
    s.treasure = pt_wave_or(m_tre);
    s.goblin = pt_wave_or(m_gob);
    s.ogre = pt_wave_or(m_ogr);
    return pass;
  }

  static __device__ __forceinline__ bool played(const int32_t *stats) {  // mdungeon_prob.py:166
    return stats[0] == 1 && stats[1] == 1;
  }
  static __device__ __forceinline__ bool too_many(const int32_t *stats) {
    return stats[2] + stats[3] + stats[4] > MD_MAX_ITEMS;
  }

  static __device__ __forceinline__ MdGame game(const MdScan &s, const int32_t *stats, int H, int W) {
    MdGame g;
    g.py = s.at_player / W + 1, g.px = s.at_player % W + 1;
    g.dy = s.at_exit / W + 1, g.dx = s.at_exit % W + 1;
    g.items = stats[2] + stats[3] + stats[4];
    g.potion = s.potion, g.treasure = s.treasure, g.goblin = s.goblin, g.ogre = s.ogre;
    return g;
  }

  // the state word's own bits: health 3 (11-13); lost is health 0
  static __device__ __forceinline__ MdState unpack(uint32_t w) { return {pt_sx(w), pt_sy(w), (int)((w >> 11) & 7)}; }
  static __device__ __forceinline__ uint32_t pack(const MdState &s) {
    return (uint32_t)s.x | ((uint32_t)s.y << 6) | ((uint32_t)s.health << 11) | ((uint32_t)(s.health <= 0) << 14);
  }

  static __device__ __forceinline__ MdState root(const MdGame &g) { return {g.px, g.py, MD_MAX_HEALTH}; }
  static __device__ __forceinline__ bool wins(const MdGame &g, const MdState &s) { return s.x == g.dx && s.y == g.dy; }
  static __device__ __forceinline__ uint32_t tag(const MdState &s) {
    return 0x80000000u | (uint32_t)s.x | ((uint32_t)s.y << 6) | ((uint32_t)s.health << 11);
  }

  // State.getHeuristic (engine.py:285-289); the collected treasures are those of the level that are no longer on the map
  static __device__ __forceinline__ int heuristic(const MdGame &g, const MdState &s, uint64_t left) {
    return abs(s.x - g.dx) + abs(s.y - g.dy) + 4 * (MD_MAX_HEALTH - s.health) - 4 * __popcll(g.treasure & ~left);
  }

  // State.update (engine.py:254-270) for direction a of 0..3 = left, right, up, down
  static __device__ __forceinline__ MdState step(const MdLds &L, const MdGame &g, const MdState &s, const PtRows &r,
                                                 uint64_t &left, int a) {
    const int tx = s.x + (a == 0 ? -1 : a == 1 ? 1 : 0), ty = s.y + (a == 2 ? -1 : a == 3 ? 1 : 0);
    MdState c = s;
    if (!pt_solid(a == 2 ? r.above : a == 3 ? r.below : r.here, tx)) {
      c.x = tx, c.y = ty;
      // updatePlayer (engine.py:229-252): a cell holds one item, so the order of its three tests does not show
      const uint32_t o = L.ord[ty * PT_LW + tx];
      if (o < 64 && ((left >> o) & 1ull)) {
        const uint64_t bit = 1ull << o;
        left &= ~bit;
        if (g.potion & bit) c.health = min(c.health + 2, MD_MAX_HEALTH);
        else if (g.goblin & bit) c.health = max(c.health - 1, 0);
        else if (g.ogre & bit) c.health = max(c.health - 2, 0);
      }
    }
    return c;
  }

  // col-potions, col-treasures and col-enemies, which are also play columns, after the health
  static __device__ __forceinline__ void finish(const MdGame &g, uint4 nd, int32_t *stats, int32_t *pc) {
    const uint64_t gone = ~pt_nleft(nd);
    stats[6] = pc[3] = __popcll(g.potion & gone);
    stats[7] = pc[4] = __popcll(g.treasure & gone);
    stats[8] = pc[5] = __popcll((g.goblin | g.ogre) & gone);
    pc[2] = unpack(nd.x).health;
  }
};

__global__ __launch_bounds__(64) void mdungeon_kernel(const PtArgs a) {
  __shared__ MdLds L;
  pt_level<MdPolicy>(a, L);
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
