// paths/pcgrl_paths.h -- solution paths of binary and zelda maps on the device (include/pcgrl_amd_paths.h): the ordered
// cell list the reference keeps for rendering, cell for cell, and the path mask.
//
// The rules (cells are (row, col) = the reference's [y, x]; d = 4-neighbour BFS distance inside the passable set):
//   trace(d, start)   empty if start is unreachable; else start, then repeatedly the first neighbour in the order up, left,
//                     right, down whose distance is one less, down to distance 0 (helper.py:321-426 get_path_coords: the
//                     np.where order of its ADJ_FILTER mask).
//   binary            helper.py:255-276 calc_longest_path(get_path=True) over "empty": components in row-major order of their
//                     first cell; per component BFS from the first cell, far = first row-major cell of the greatest distance,
//                     BFS from far, L = its greatest distance; the winner is the first component whose L is strictly greater
//                     than every earlier one; L == 0: no path; else trace(d_far, first row-major cell with d_far == L): L + 1
//                     cells from the far end back to far.
//   zelda             zelda_ctrl_prob.py:153-165 (render_path): nothing unless exactly one player, key and door; A =
//                     trace(BFS from the player over everything but solid and door, key), B = trace(BFS from the key over
//                     everything but solid, door); the path is A then B without the cells of player, key and door.
//
// One kernel template, the engine's mapping: LPE lanes per map, one lane per map row, row masks in VGPRs, 64 / LPE maps per
// wavefront, one wavefront per workgroup.  A BFS level is bfs_level (pcgrl_kernels2d.h); the cells a level newly reaches get
// the level number in a per-map table in LDS (uint16, n_cells entries: 512 B at 16 x 16, 8 KB at 64 x 64) -- nothing of the
// distances goes through HBM.
//   binary   component_fars gives every component's far cell; ONE recorded multi-source BFS from all of them fills the table
//            with every component's d_far at once (components are disjoint), and its last frontier holds the end cells of the
//            components that attain the maximum.  The winner among those is the one whose first cell comes first: the first
//            row-major cell of their union (one flood) lies in it, a second flood cuts it out.
//   zelda    the table is used twice: BFS from the player, trace from the key; BFS from the key, trace from the door.  A
//            recorded BFS stops at the end of the trip in which it reaches its target.
// The back-trace is a dependent chain of LDS reads, one step per path cell (at most n_cells for binary; the longest known at
// 64 x 64 is a one-cell-wide spiral's 2 111, about 0.1 ms; zelda's two halves on a serpentine: 3 116 of 2 * n_cells): every
// lane of the group walks it (the reads are broadcasts), the four neighbour reads of a step are issued together, lane i of
// the group keeps the cell of step i mod LPE and the group stores LPE cells with one instruction; the (-1, -1) fill and the
// overlay rows are written by all lanes in parallel.  Plain vector stores only.
#pragma once
#include <hip/hip_runtime.h>

#include "../pcgrl_common.h"

namespace pcgrl {

struct PathArgs {
  int16_t *path;     // [n][cap][2] (row, col); rows from min(len, cap) on are (-1, -1)
  int32_t *len;      // [n] the full length, also beyond cap
  uint8_t *overlay;  // [n][H][W] 1 on path cells, or null
  int32_t cap;
  int32_t from_grids;  // 0: the maps are the engine's planes; 1: Params::init_grids, uint8 [n][H][W]
  int32_t ts;          // filled in by launch_paths: entries of one map's distance table (n_cells rounded up to 8)
};

// one per translation unit (the six (LPE, M) forms validate() can choose, each from planes and from caller bytes)
hipError_t launch_paths_binary(const Params &p, int lpe, const PathArgs &a, hipStream_t s);
hipError_t launch_paths_zelda(const Params &p, int lpe, const PathArgs &a, hipStream_t s);

// Params::n_envs maps (the engine's own, or a.from_grids) -> a.path / a.len / a.overlay
inline hipError_t launch_paths(const Params &p, int lpe, const PathArgs &args, hipStream_t s) {
  PathArgs a = args;
  a.ts = (p.cfg.dims[0] * p.cfg.dims[1] + 7) & ~7;
  switch (p.cfg.problem) {
    case PCGRL_PROB_BINARY: return launch_paths_binary(p, lpe, a, s);
    case PCGRL_PROB_ZELDA: return launch_paths_zelda(p, lpe, a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace pcgrl

#ifdef PCGRL_KERNEL_TU
#include "../pcgrl_kernels2d.h"

namespace pcgrl {

constexpr uint32_t PATH_UNREACHED = 0xFFFFu;
constexpr uint32_t PATH_NO_CELL = 0xFFFFFFFFu;  // a packed cell that no map cell equals: (-1, -1)
constexpr int PATH_SWEEP_UNROLL = 4;

__device__ inline uint32_t pack_cell(int r, int c) { return (uint32_t)r | ((uint32_t)c << 16); }  // int16 (row, col) in memory

// the group's whole table to "unreached" (ts is a multiple of 8 entries)
template <int LPE>
__device__ inline void table_clear(const Grp<LPE> &g, uint16_t *tab, int ts) {
  uint32_t *t32 = (uint32_t *)tab;
  for (int i = g.row; i < ts / 2; i += LPE) t32[i] = 0xFFFFFFFFu;
}

template <typename M>
__device__ inline void put_levels(uint16_t *row_tab, M cells, int lev) {
  while (cells) {
    row_tab[ctz_m(cells)] = (uint16_t)lev;
    cells &= cells - M(1);
  }
}

// sweep() (pcgrl_kernels2d.h) with the levels written down: level-synchronous BFS from `src` inside `avail`, every cell's
// level into the lane's row of the table.  len = number of levels, last = the cells of the final level.  A group with a
// `stop` cell is finished at the end of the trip in which it reaches it (every level below the cell's own is complete then).
template <int LPE, typename M>
__device__ inline void sweep_record(const Grp<LPE> &g, M src, M avail, M stop, uint16_t *row_tab, int &len, M &last) {
  M front = src & avail;
  M free_cells = avail & ~front;
  put_levels(row_tab, front, 0);
  const bool has_stop = g.gany(stop != 0);
  M mynb = M(0);
  int mylev = 0, lev = 0;
  while (true) {
#pragma unroll
    for (int u = 0; u < PATH_SWEEP_UNROLL; u++) {
      const M nb = bfs_level(g, front, free_cells);
      lev++;
      put_levels(row_tab, nb, lev);
      mylev = nb ? lev : mylev;
      mynb = nb ? nb : mynb;
      front = nb;
    }
    const bool alive = g.gany(front != 0);
    const bool reached = has_stop && g.gany((stop & avail & ~free_cells) != 0);
    if (__ballot(alive && !reached) == 0) break;
  }
  len = (int)g.gmax((uint32_t)mylev);
  last = (len > 0 && mylev == len) ? mynb : M(0);
}

// the (row, col) of a one-cell set, in every lane of the group; false (and 0, 0) for the empty set
template <int LPE, typename M>
__device__ inline bool cell_of(const Grp<LPE> &g, M x, int &r, int &c) {
  const uint64_t gb = g.gballot(x != 0);
  r = gb ? __builtin_ctzll(gb) : 0;
  c = (int)g.gbcast(x ? (uint32_t)ctz_m(x) : 0u, r);
  return gb != 0;
}

// the output cursor of one map: lane i of the group keeps the cell of step i mod LPE, a full set goes out in one store
template <int LPE>
struct PathOut {
  int16_t *dst;  // this map's [cap][2]
  int cap, n;
  bool aligned;  // 4-byte aligned rows: one dword per cell
  uint32_t mine;
  __device__ inline void put(int i, uint32_t v) const {
    if (i >= cap) return;
    if (aligned) {
      ((uint32_t *)dst)[i] = v;
    } else {
      dst[2 * i] = (int16_t)(v & 0xFFFFu);
      dst[2 * i + 1] = (int16_t)(v >> 16);
    }
  }
  __device__ inline void emit(const Grp<LPE> &g, bool on, uint32_t cell) {
    const int slot = n & (LPE - 1);
    mine = (on && slot == g.row) ? cell : mine;
    if (on && slot == LPE - 1) put(n - (LPE - 1) + g.row, mine);
    n += on ? 1 : 0;
  }
  // the cells of the last, partial set, then (-1, -1) up to cap
  __device__ inline void finish(const Grp<LPE> &g, bool active) {
    if (!active) return;
    const int part = n & (LPE - 1);
    if (g.row < part) put(n - part + g.row, mine);
    for (int i = n + g.row; i < cap; i += LPE) put(i, PATH_NO_CELL);
  }
};

// trace(d, start) from the table: `on` groups start at (r, c); the cells equal to skip0 / skip1 / skip2 are walked but not
// emitted.  ov collects the lane's row of the overlay.
template <int LPE, typename M>
__device__ inline void trace(const Grp<LPE> &g, const uint16_t *tab, int H, int W, bool on, int r, int c, uint32_t skip0,
                             uint32_t skip1, uint32_t skip2, PathOut<LPE> &out, M &ov) {
  r = on ? r : 0;
  c = on ? c : 0;
  uint32_t d = tab[r * W + c];
  on = on && d != PATH_UNREACHED;
  while (__ballot(on) != 0) {
    const uint32_t cell = pack_cell(r, c);
    const bool keep = on && cell != skip0 && cell != skip1 && cell != skip2;
    out.emit(g, keep, cell);
    ov |= (keep && g.row == r) ? (M(1) << c) : M(0);
    // the four neighbours at once (a neighbour outside the map reads the cell itself, which is not one less)
    const int at = r * W + c;
    const uint32_t up = tab[r > 0 ? at - W : at], left = tab[c > 0 ? at - 1 : at];
    const uint32_t right = tab[c + 1 < W ? at + 1 : at], down = tab[r + 1 < H ? at + W : at];
    const uint32_t want = d - 1u;  // (d == 0: 0xFFFFFFFF, no 16-bit entry equals it)
    on = on && d != 0;
    if (on) {
      if (up == want) r--;
      else if (left == want) c--;
      else if (right == want) c++;
      else if (down == want) r++;
      else on = false;  // (cannot happen: every reached cell but the source has a neighbour one level below)
      d = want;
    }
  }
}

template <int PROB, int LPE, typename M, bool GRIDS>
__global__ __launch_bounds__(64) void paths_kernel(Params p, PathArgs a) {
  constexpr int NB = ProbTraits<PROB>::NB, EPW = 64 / LPE;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  Grp<LPE> g;
  g.init();
  const int H = p.cfg.dims[0], W = p.cfg.dims[1];
  const int env = blockIdx.x * EPW + (g.lane / LPE);
  const bool active = env < p.n_envs;
  const int e = active ? env : 0;
  const bool rowok = active && g.row < H;
  const M colmask = rowok ? (W >= (int)(8 * sizeof(M)) ? ~M(0) : ((M(1) << W) - M(1))) : M(0);
  M b[NB];
  if constexpr (GRIDS) {  // caller bytes, as stats_for_grids_kernel reads them
#pragma unroll
    for (int k = 0; k < NB; k++) b[k] = 0;
    if (rowok) {
      const uint8_t *src = p.init_grids + ((size_t)e * H + g.row) * W;
      for (int x = 0; x < W; x++) {
        const int t = src[x];
#pragma unroll
        for (int k = 0; k < NB; k++) b[k] |= (M)((t >> k) & 1) << x;
      }
    }
  } else {
    load_planes<NB, M>(p, e, g.row, rowok, b);
  }
  uint16_t *tab = (uint16_t *)lds + (size_t)(g.lane / LPE) * a.ts;  // this map's distances
  uint16_t *row_tab = tab + g.row * W;                                // (only lanes with a map row write through it)
  PathOut<LPE> out;
  out.dst = a.path + (size_t)e * (size_t)a.cap * 2;
  out.cap = a.cap;
  out.n = 0;
  out.aligned = ((uintptr_t)a.path & 3u) == 0;
  out.mine = PATH_NO_CELL;
  M ov = M(0);
  table_clear(g, tab, a.ts);
  __syncthreads();
  if constexpr (PROB == PCGRL_PROB_BINARY) {
    const M pass = ~b[0] & colmask;
    const M fars = component_fars(g, pass);
    int L;
    M last;
    sweep_record(g, fars, pass, M(0), row_tab, L, last);
    // the components that attain L, the one of them whose first cell comes first, its first end cell
    const M attain = flood(g, last, pass);
    const M winner = flood(g, first_rowmajor(g, attain), pass);
    const M end = first_rowmajor(g, (M)(last & winner));
    int r, c;
    const bool on = cell_of(g, end, r, c);
    __syncthreads();
    trace(g, tab, H, W, on, r, c, PATH_NO_CELL, PATH_NO_CELL, PATH_NO_CELL, out, ov);
  } else {
    static_assert(PROB == PCGRL_PROB_ZELDA, "paths: binary and zelda");
    // ids: 0 empty 1 solid 2 player 3 key 4 door 5 bat 6 scorpion 7 spider
    const M solid = b[0] & ~b[1] & ~b[2] & colmask, door = ~b[0] & ~b[1] & b[2] & colmask;
    const M player = ~b[0] & b[1] & ~b[2] & colmask, key = b[0] & b[1] & ~b[2] & colmask;
    const M walk = colmask & ~(solid | door), walkd = colmask & ~solid;
    const uint32_t c01 = g.gsum((uint32_t)popc_m(player) | ((uint32_t)popc_m(key) << 16));
    const uint32_t c2 = g.gsum((uint32_t)popc_m(door));
    const bool want = c01 == 0x00010001u && c2 == 1u;
    int pr, pc, kr, kc, dr, dc, len;
    M last;
    cell_of(g, want ? player : M(0), pr, pc);
    cell_of(g, want ? key : M(0), kr, kc);
    cell_of(g, want ? door : M(0), dr, dc);
    const uint32_t sp = want ? pack_cell(pr, pc) : PATH_NO_CELL, sk = want ? pack_cell(kr, kc) : PATH_NO_CELL;
    const uint32_t sd = want ? pack_cell(dr, dc) : PATH_NO_CELL;
    sweep_record(g, want ? player : M(0), walk, want ? key : M(0), row_tab, len, last);
    __syncthreads();
    trace(g, tab, H, W, want, kr, kc, sp, sk, sd, out, ov);
    __syncthreads();
    table_clear(g, tab, a.ts);
    __syncthreads();
    sweep_record(g, want ? key : M(0), walkd, want ? door : M(0), row_tab, len, last);
    __syncthreads();
    trace(g, tab, H, W, want, dr, dc, sp, sk, sd, out, ov);
  }
  out.finish(g, active);
  if (active && g.row == 0) a.len[env] = out.n;
  if (a.overlay != nullptr && rowok) {
    uint8_t *dst = a.overlay + ((size_t)env * H + g.row) * W;
    int x = 0;
    if (((uintptr_t)dst & 3u) == 0)
      for (; x + 4 <= W; x += 4) *(uint32_t *)(dst + x) = spread4(nibble_at<M>(ov, x));
    for (; x < W; x++) dst[x] = (uint8_t)((ov >> x) & M(1));
  }
}

template <int PROB, int LPE, typename M>
static hipError_t launch_paths_pl(const Params &p, const PathArgs &a, hipStream_t s) {
  constexpr int EPW = 64 / LPE;
  const dim3 grid((p.n_envs + EPW - 1) / EPW), block(64);
  const size_t lds = (size_t)EPW * a.ts * sizeof(uint16_t);  // <= 8 KB
  if (a.from_grids)
    hipLaunchKernelGGL((paths_kernel<PROB, LPE, M, true>), grid, block, lds, s, p, a);
  else
    hipLaunchKernelGGL((paths_kernel<PROB, LPE, M, false>), grid, block, lds, s, p, a);
  return hipGetLastError();
}

template <int PROB>
static hipError_t launch_paths_prob(const Params &p, int lpe, const PathArgs &a, hipStream_t s) {
  if (p.n_envs <= 0) return hipSuccess;
  if (p.cfg.dims[1] > 32) {  // 64-bit row masks: 32 or 64 lanes per map (validate())
    if (lpe == 32) return launch_paths_pl<PROB, 32, uint64_t>(p, a, s);
    return launch_paths_pl<PROB, 64, uint64_t>(p, a, s);
  }
  switch (lpe) {
    case 8: return launch_paths_pl<PROB, 8, uint32_t>(p, a, s);
    case 16: return launch_paths_pl<PROB, 16, uint32_t>(p, a, s);
    case 32: return launch_paths_pl<PROB, 32, uint32_t>(p, a, s);
    default: return launch_paths_pl<PROB, 64, uint32_t>(p, a, s);
  }
}

}  // namespace pcgrl
#endif
