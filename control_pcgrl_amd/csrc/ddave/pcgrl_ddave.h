// ddave/pcgrl_ddave.h -- Dangerous Dave levels on the device (include/pcgrl_amd_ddave.h): what DDaveProblem.get_stats computes
// for an H x W map of 7 tile types (envs/probs/ddave/ddave_prob.py:149-169) -- seven map statistics and the four-stage
// play-through of ddave/engine.py.  DESIGN.md section 31 has the rules with every quirk; tests/ddave_rules.py is the same in
// plain Python.
//
// ddave_kernel: one 64-lane wave per level, pt_level<DdPolicy> of playthrough/pcgrl_playthrough.h.  That header has the kernel's
// layout, the search loop, the open list, the visited set, the region count and the workspace; this one has what is Dave's:
//   scans     a lane counts the tiles of cells lane, lane + 64, ... and walks down from each player tile for dist-floor; lane
//             r < H builds row r's masks (solid, spike, diamond).  The regions are everything but solid and spike.
//   level     spike[y] bit rows beside the shared solid[y] and ord[y][x] (the diamonds' ordinals); the player, key and door
//             positions in registers.
//   node      DdState: the state word's own bits are airTime 2 (bits 11-12) | col_key 1 (bit 13) | jumps 14 (bits 17-30).  The
//             visited tag is x, y, col_key and an occupied bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../measures/pcgrl_measures_wave.h"  // MeasWaveArgs, meas_wave_map
#include "../playthrough/pcgrl_playthrough.h"  // PtArgs, the workspace, pt_level

namespace pcgrl {

constexpr int DD_TILES = 7;
constexpr int DD_STATS = PT_STATS;  // player, dist-floor, exit, diamonds, key, spikes, regions, num-jumps, col-diamonds, dist-win, sol-length
constexpr int DD_MAX_H = PT_MAX_H, DD_MAX_W = PT_MAX_W;
constexpr int DD_MAX_CELLS = DD_MAX_H * DD_MAX_W;  // 512
constexpr int DD_MAX_DIAMONDS = 64;  // the remaining diamonds are a node's one 64-bit word
// 2 * heuristic >= -2 * 5 * 64; 2 * heuristic + 2 * depth + bias <= 2 * (31 + 15 + 52) + 32 000 + 640 < 2^16
constexpr int DD_F_BIAS = 2 * 5 * DD_MAX_DIAMONDS;
constexpr int DD_MEAS_TILES = 7, DD_MEAS_PLANES = 3;

hipError_t launch_ddave(const PtArgs &a, hipStream_t s);
hipError_t launch_dd_measures(const MeasWaveArgs &a, hipStream_t s);

#ifdef PCGRL_DD_KERNEL  // (ddave/pcgrl_k_ddave.hip has it, with PCGRL_PT_KERNEL)

struct DdLds {
  uint8_t map[DD_MAX_CELLS];
  uint64_t solid[PT_LH], spike[PT_LH];
  uint8_t ord[PT_LH * PT_LW];
};

// what the search reads besides the LDS level (lane 0's registers)
struct DdGame {
  int px, py, kx, ky, dx, dy;  // bordered coordinates
  int wh;                      // (W + 2) + (H + 2): State.width + State.height
  int items;                   // diamonds in the level, <= 64
};

// where the player, the door and the key are: the last cell of each (the game needs exactly one)
struct DdScan {
  int at_player, at_exit, at_key;
};

struct DdState {
  int x, y, air, key, lost, jumps;
};

struct DdPolicy {
  using Lds = DdLds;
  using Game = DdGame;
  using Scan = DdScan;
  using State = DdState;
  static constexpr int TILES = DD_TILES, REGIONS = 6, F_BIAS = DD_F_BIAS;

  static __device__ __forceinline__ uint32_t scan(DdLds &L, int H, int W, int32_t *stats, int32_t *pc, DdScan &s) {
    const int lane = threadIdx.x, cells = H * W;
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
    stats[0] = pt_wave_sum(cnt_player);
    stats[1] = pt_wave_sum(dist_floor);
    stats[2] = pt_wave_sum(cnt_exit);
    stats[3] = pt_wave_sum(cnt_diamond);
    stats[4] = pt_wave_sum(cnt_key);
    stats[5] = pt_wave_sum(cnt_spike);
    pc[5] = stats[3];
    s.at_player = pt_wave_max(at_player);
    s.at_exit = pt_wave_max(at_exit);
    s.at_key = pt_wave_max(at_key);

    // lane r < H: row r's masks and its rows of the bordered level
    uint32_t pass = 0, solid = 0, spike = 0, dia = 0;
    if (lane < H)
      for (int c = 0; c < W; c++) {
        const int t = L.map[lane * W + c];
        solid |= (uint32_t)(t == 1) << c;
        spike |= (uint32_t)(t == 6) << c;
        dia |= (uint32_t)(t == 4) << c;
      }
    if (lane < H) pass = ~(solid | spike) & (W == 32 ? ~0u : (1u << W) - 1u);
    pt_level_rows(L.solid, L.ord, H, W, solid, dia);
    if (lane < H) L.spike[lane + 1] = (uint64_t)spike << 1;
    else if (lane < H + 2) L.spike[lane == H ? 0 : H + 1] = 0;
    return pass;
  }

  static __device__ __forceinline__ bool played(const int32_t *stats) {  // ddave_prob.py:164-165
    return stats[0] == 1 && stats[2] == 1 && stats[4] == 1;
  }
  static __device__ __forceinline__ bool too_many(const int32_t *stats) { return stats[3] > DD_MAX_DIAMONDS; }

  static __device__ __forceinline__ DdGame game(const DdScan &s, const int32_t *stats, int H, int W) {
    DdGame g;
    g.py = s.at_player / W + 1, g.px = s.at_player % W + 1;
    g.ky = s.at_key / W + 1, g.kx = s.at_key % W + 1;
    g.dy = s.at_exit / W + 1, g.dx = s.at_exit % W + 1;
    g.wh = W + 2 + H + 2;
    g.items = stats[3];
    return g;
  }

  // the state word's own bits: airTime 2 (11-12) | col_key 1 (13) | jumps 14 (17-30)
  static __device__ __forceinline__ DdState unpack(uint32_t w) {
    return {pt_sx(w), pt_sy(w), (int)((w >> 11) & 3), (int)((w >> 13) & 1), pt_slost(w), (int)((w >> 17) & 0x3FFF)};
  }
  static __device__ __forceinline__ uint32_t pack(const DdState &s) {
    return (uint32_t)s.x | ((uint32_t)s.y << 6) | ((uint32_t)s.air << 11) | ((uint32_t)s.key << 13) | ((uint32_t)s.lost << 14) |
           ((uint32_t)s.jumps << 17);
  }

  static __device__ __forceinline__ DdState root(const DdGame &g) { return {g.px, g.py, 0, 0, 0, 0}; }
  static __device__ __forceinline__ bool wins(const DdGame &g, const DdState &s) { return s.key && s.x == g.dx && s.y == g.dy; }
  static __device__ __forceinline__ uint32_t tag(const DdState &s) {
    return 0x80000000u | (uint32_t)s.x | ((uint32_t)s.y << 6) | ((uint32_t)s.key << 11);
  }

  // State.getHeuristic (engine.py:278-283)
  static __device__ __forceinline__ int heuristic(const DdGame &g, const DdState &s, uint64_t left) {
    const int dist = s.key ? abs(s.x - g.dx) + abs(s.y - g.dy) : abs(s.x - g.kx) + abs(s.y - g.ky) + g.wh;
    return dist - 5 * (g.items - __popcll(left));
  }

  // State.update (engine.py:229-264) for direction a of 0..3 = stay, left, right, jump
  static __device__ __forceinline__ DdState step(const DdLds &L, const DdGame &g, const DdState &s, const PtRows &r,
                                                 uint64_t &left, int a) {
    DdState c = {s.x, s.y, s.air, s.key, 0, s.jumps};
    if (a == 1 || a == 2) {
      const int tx = a == 1 ? s.x - 1 : s.x + 1;
      if (!pt_solid(r.here, tx)) c.x = tx;
    } else if (a == 3) {
      if (pt_solid(r.below, s.x) && !pt_solid(r.above, s.x)) {  // on the ground, under no ceiling
        c.air = 3;
        c.jumps++;
      }
    }
    if (c.air > 1) {
      c.air--;
      if (!pt_solid(r.above, c.x)) c.y--;
      else c.air = 1;
    } else if (c.air == 1) {
      c.air = 0;
    } else if (!pt_solid(r.below, c.x)) {
      c.y++;
    }
    // updatePlayer (engine.py:212-227): a diamond, else a spike, else the key
    const uint32_t o = L.ord[c.y * PT_LW + c.x];
    if (o < 64 && ((left >> o) & 1ull)) left &= ~(1ull << o);
    else if ((L.spike[c.y] >> c.x) & 1u) c.lost = 1;
    else if (!c.key && c.x == g.kx && c.y == g.ky) c.key = 1;
    return c;
  }

  // num-jumps and col-diamonds; the play columns airTime, health, col_key (scan has set the level's diamonds)
  static __device__ __forceinline__ void finish(const DdGame &g, uint4 nd, int32_t *stats, int32_t *pc) {
    const DdState s = unpack(nd.x);
    stats[7] = s.jumps;
    stats[8] = g.items - __popcll(pt_nleft(nd));
    pc[2] = s.air, pc[3] = 1 - s.lost, pc[4] = s.key;
  }
};

__global__ __launch_bounds__(64) void ddave_kernel(const PtArgs a) {
  __shared__ DdLds L;
  pt_level<DdPolicy>(a, L);
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
