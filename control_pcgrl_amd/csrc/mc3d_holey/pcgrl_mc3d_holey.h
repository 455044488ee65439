// mc3d_holey/pcgrl_mc3d_holey.h -- the 3-D holey dungeon and maze levels on the device (include/pcgrl_amd_mc3d_holey.h): what
// Minecraft3DholeyDungeonProblem.get_stats and Minecraft3DholeymazeProblem.get_stats compute on the bordered map with its two
// holes -- the AIR regions, the tile counts and the routes of helper_3D.run_dijkstra under the player physics of
// helper_3D._passable -- and the loss ControlWrapper.get_loss would derive from them.  DESIGN.md section 36 has the rules with
// every quirk; tests/mc3d_holey_rules.py is the same in plain Python.  The move rule is restated here (h3_move): nothing of
// pcgrl_kernels3d.h is included, so no existing kernel's code changes.
//
// mc3d_holey_kernel: one workgroup of two waves per level, the grid striding over the levels (one workspace slot per block).
//   map       the bordered level, (Z + 2)(Y + 2)(X + 2) <= 18^3 bytes, is built in LDS from byte loads (any alignment): DIRT
//             border, the four hole cells AIR; an id the problem does not know becomes DIRT and raises error bit 0.
//   planes    col[y][x]: bit z = the cell is passable (every test of the move rule is a bit test on three such words: the own
//             column, the neighbour's, the landing's); air[z][y]: bit x = AIR, the rows the regions are flooded over.
//   regions   AIR cells without an AIR neighbour are counted and removed at once; the rest is peeled a region at a time, every
//             thread growing its rows (z, y) from the rows (z, y +- 1), (z +- 1, y) and along x until nothing changes (double
//             buffered, one barrier per sweep).
//   search    lane 0 of wave 0 runs the search from the entrance, lane 0 of wave 1 the dungeon's search from the first chest:
//             they are independent.  The queue is a ring of 64-bit entries (cell 13 | length 15 | jumps 13 | parent 13 |
//             move 5) in the block's workspace slot; an entry that the cell's accepted length already beats is dropped when it
//             would be pushed (exact: that length only shrinks) and again when it is popped (the reference's test).  Per cell
//             the accepted length (0 = not a key of `paths`), jump count, parent, move kind and the ordinal of the first
//             acceptance: in LDS up to 1024 bordered cells (interiors up to 8^3), else in the workspace slot.
//   ring      Q = the power of two >= 8 * cells entries.  The live entries belong to two consecutive depths (numbers of moves
//             from the start): the rest of depth k and what depth k's accepted pops have pushed, at most four each.  Were no
//             cell accepted twice within one depth, that is 4 * cells + 4 * cells.  A cell can be accepted again within a depth
//             (ever shorter lengths arriving in queue order), so this is a capacity and not a proof: a push that finds the ring
//             full ends the level with error bit 2 (ERR_QUEUE), statistics -1 and loss -inf.
//   routes    the accepted parent chain is consistent when the queue is empty (a cell accepted again pushes its successors
//             again, and they are accepted again), so a route is read back from its end along parent and move kind -- the move
//             gives the traversed tiles -- and stored forwards, the position counted down from the accepted length.  The same
//             walk sets the route's bits in an LDS plane: remove_stacked_path_tiles keeps a tile when the tile below it is not
//             in the route, one AND-NOT per row.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcgrl {

constexpr int H3_MAX = 16, H3_B = H3_MAX + 2;
constexpr int H3_MAX_CELLS = H3_B * H3_B * H3_B;  // 5832 < 2^13
constexpr int H3_MAX_ROWS = H3_B * H3_B;          // 324
constexpr int H3_SMALL_CELLS = 1024;              // up to here the per-cell search state lives in LDS
constexpr int H3_THREADS = 128;
constexpr int H3_MAX_STATS = 6, H3_PLAY = 12;
constexpr int H3_DUNGEON = 0, H3_MAZE = 1;
constexpr uint32_t H3_ERR_TILE = 1, H3_ERR_HOLE = 2, H3_ERR_QUEUE = 4;
constexpr int H3_START = 31;  // the move kind of a search's first cell

struct H3Args {
  int32_t problem, Z, Y, X, n;
  const uint8_t *grids;  // uint8 [n][Z][Y][X]
  const int32_t *holes;  // int32 [n][2][3]: entrance and exit foot (z, y, x), bordered
  uint8_t *ws;           // gridDim.x slots of ws_stride bytes, 16-byte aligned
  int64_t ws_stride;
  int32_t qcap;          // ring entries per search, a power of two
  int32_t route_cap;
  int32_t *stats;        // [n][6] or [n][4]
  double *loss;          // [n] or null
  int32_t *play;         // [n][12] or null
  uint32_t *error;       // [n] or null
  int16_t *coords;       // [n][route_cap][3] or null
  int32_t *route_len;    // [n] or null
  int32_t *leg_len;      // [n][2] or null
  int16_t *coords2;      // [n][route_cap][3] or null
  int32_t *route2_len;   // [n] or null
  uint8_t *overlay;      // [n][Z+2][Y+2][X+2] or null
  uint8_t *overlay2;
  double weight[H3_MAX_STATS], trg_lo[H3_MAX_STATS], trg_hi[H3_MAX_STATS];
};

__host__ __device__ inline int h3_cells(int Z, int Y, int X) { return (Z + 2) * (Y + 2) * (X + 2); }
inline int32_t h3_qcap(int cells) {
  int32_t c = 64;
  while (c < 8 * cells) c <<= 1;
  return c;
}
__host__ __device__ inline int64_t h3_align16(int64_t b) { return (b + 15) / 16 * 16; }
// one search's per-cell state in the workspace: four uint16 arrays and one uint8 array (0 when it lives in LDS)
__host__ __device__ inline int64_t h3_state_bytes(int cells) {
  return cells <= H3_SMALL_CELLS ? 0 : 4 * h3_align16(2 * (int64_t)cells) + h3_align16(cells);
}
inline int64_t h3_ws_stride(int cells) { return 2 * ((int64_t)h3_qcap(cells) * 8 + h3_state_bytes(cells)); }

hipError_t launch_mc3d_holey(const H3Args &a, int blocks, hipStream_t s);

#ifdef PCGRL_H3_KERNEL  // (mc3d_holey/pcgrl_k_mc3d_holey.hip has it)

struct H3State {
  uint16_t *len, *jmp, *par, *ord;
  uint8_t *kind;
};

struct H3Lds {
  uint32_t col[H3_MAX_ROWS];
  uint32_t air[H3_MAX_ROWS];
  uint32_t cur[2][H3_MAX_ROWS];
  uint32_t ov[2][H3_MAX_ROWS];
  uint16_t st16[2][4][H3_SMALL_CELLS];
  uint8_t st8[2][H3_SMALL_CELLS];
  uint8_t map[H3_MAX_CELLS];
  int32_t seed, singles, chest, n_chest, n_enemy, overflow, far;
  uint32_t key_near, key_far;
  int32_t acc[2], pushed[2];
  int32_t rlen[2], legs[2], kept[2];
};

struct H3Dims {
  int BZ, BY, BX;
};

__device__ __forceinline__ int h3_cell(const H3Dims &d, int x, int y, int z) { return (z * d.BY + y) * d.BX + x; }
__device__ __forceinline__ bool h3_bit(uint32_t c, int z) { return z >= 0 && z < 32 && ((c >> z) & 1u); }

// helper_3D._passable (:214-319) for one direction d (0 +x, 1 +y, 2 -x, 3 -y): the first matching rule of the elif chain.
// kind: 0 walk, 1 step down, 2 step up, 3 / 4 / 5 jump landing level / one up / one down; add = tiles the move appends.
__device__ __forceinline__ bool h3_move(const H3Lds &L, const H3Dims &dm, int x, int y, int z, int d, int &nx, int &ny, int &nz,
                                        int &add, int &kind) {
  const int dx = d == 0 ? 1 : (d == 2 ? -1 : 0), dy = d == 1 ? 1 : (d == 3 ? -1 : 0);
  const int ax = x + dx, ay = y + dy;
  if (ax < 0 || ay < 0 || ax >= dm.BX || ay >= dm.BY) return false;
  const uint32_t own = L.col[y * dm.BX + x], c = L.col[ay * dm.BX + ax];
  const bool p0 = h3_bit(c, z), p1 = h3_bit(c, z + 1), p2 = h3_bit(c, z + 2), m1 = h3_bit(c, z - 1), m2 = h3_bit(c, z - 2);
  nx = ax, ny = ay;
  if ((z == 0 || (z > 0 && !m1)) && p0 && p1) {
    nz = z, add = 1, kind = 0;
    return true;
  }
  if ((z - 1 == 0 || (z - 1 > 0 && !m2)) && m1 && p0 && p1) {
    nz = z - 1, add = 2, kind = 1;
    return true;
  }
  if (z + 2 < dm.BZ && !p0 && p1 && p2 && h3_bit(own, z + 2)) {
    nz = z + 1, add = 2, kind = 2;
    return true;
  }
  const int jx = x + 2 * dx, jy = y + 2 * dy;
  if (z - 2 >= 0 && z + 2 < dm.BZ && p2 && p1 && p0 && m1 && m2 && h3_bit(own, z + 2) && jx >= 0 && jy >= 0 && jx < dm.BX &&
      jy < dm.BY) {
    const uint32_t j = L.col[jy * dm.BX + jx];
    nx = jx, ny = jy;
    if (h3_bit(j, z + 1) && h3_bit(j, z + 2) && h3_bit(j, z) && !h3_bit(j, z - 1)) {
      nz = z, add = 2, kind = 3;
      return true;
    }
    if (z + 3 < dm.BZ && h3_bit(j, z + 3) && h3_bit(j, z + 2) && h3_bit(j, z + 1) && !h3_bit(j, z)) {
      nz = z + 1, add = 3, kind = 4;
      return true;
    }
    if (h3_bit(j, z) && h3_bit(j, z + 1) && h3_bit(j, z - 1) && !h3_bit(j, z - 2)) {
      nz = z - 1, add = 3, kind = 5;
      return true;
    }
  }
  return false;
}

__device__ __forceinline__ uint64_t h3_pack(int cell, int len, int jumps, int parent, int kind) {
  return (uint64_t)cell | ((uint64_t)len << 13) | ((uint64_t)jumps << 28) | ((uint64_t)parent << 41) | ((uint64_t)kind << 54);
}

// helper_3D.run_dijkstra (:422-490) by one lane.  st.len must be zero on entry.
__device__ inline void h3_search(const H3Lds &L, const H3Dims &dm, const H3State &st, uint64_t *q, uint32_t qmask, int start,
                                 int &accepted, int &pushed, bool &overflow) {
  const int cells = dm.BZ * dm.BY * dm.BX;
  uint32_t head = 0, tail = 1;
  int first = 0;
  accepted = 0, pushed = 1, overflow = false;
  q[0] = h3_pack(start, 1, 0, start, H3_START);
  while (head != tail) {
    const uint64_t e = q[head & qmask];
    head++;
    const int cell = (int)(e & 0x1FFFu), len = (int)((e >> 13) & 0x7FFFu), jumps = (int)((e >> 28) & 0x1FFFu);
    if (cell >= cells) continue;  // never: the ring holds what this lane packed
    const int old = st.len[cell];
    if (old > 0 && old <= len) continue;
    const int x = cell % dm.BX, y = (cell / dm.BX) % dm.BY, z = cell / (dm.BX * dm.BY);
    if (z + 1 == dm.BZ || !h3_bit(L.col[y * dm.BX + x], z + 1)) continue;  // no head-room: marked, never a key of paths
    if (old == 0) st.ord[cell] = (uint16_t)first++;
    st.len[cell] = (uint16_t)len;
    st.jmp[cell] = (uint16_t)jumps;
    st.par[cell] = (uint16_t)((e >> 41) & 0x1FFFu);
    st.kind[cell] = (uint8_t)((e >> 54) & 0x1Fu);
    accepted++;
    for (int d = 0; d < 4; d++) {
      int nx, ny, nz, add, kind;
      if (!h3_move(L, dm, x, y, z, d, nx, ny, nz, add, kind)) continue;
      pushed++;
      const int nc = h3_cell(dm, nx, ny, nz), nl = len + add;
      if (nz < 0 || nz >= dm.BZ) continue;  // never: the rule's own guards
      const int ol = st.len[nc];
      if (ol > 0 && ol <= nl) continue;
      if (tail - head > qmask) {
        overflow = true;
        return;
      }
      q[tail & qmask] = h3_pack(nc, nl, jumps + (kind >= 3 ? 1 : 0), cell, kind | (d << 3));
      tail++;
    }
  }
}

// The route that ends on `target` (accepted by the search of `st`), read back along the parent chain: its tiles go to
// coords[base + i] for i below the accepted length (only positions below cap are written) and into the bit plane `ov`.
__device__ inline void h3_walk(const H3Dims &dm, const H3State &st, int target, int base, int16_t *coords, int cap, uint32_t *ov) {
  int pos = base + (int)st.len[target] - 1;
  int c = target;
  const int cells = dm.BZ * dm.BY * dm.BX;
  auto put = [&](int x, int y, int z) {
    if (pos >= 0) {
      if (coords && pos < cap) {
        coords[pos * 3 + 0] = (int16_t)x;
        coords[pos * 3 + 1] = (int16_t)y;
        coords[pos * 3 + 2] = (int16_t)z;
      }
      if (z >= 0 && z < dm.BZ) ov[z * dm.BY + y] |= 1u << x;
    }
    pos--;
  };
  for (int guard = 0; guard < cells; guard++) {
    const int x = c % dm.BX, y = (c / dm.BX) % dm.BY, z = c / (dm.BX * dm.BY);
    put(x, y, z);
    const int k = st.kind[c];
    if (k == H3_START) break;
    const int p = st.par[c];
    if (p >= cells) break;
    const int px = p % dm.BX, py = (p / dm.BX) % dm.BY, pz = p / (dm.BX * dm.BY);
    const int d = k >> 3, kk = k & 7;
    const int ax = px + (d == 0 ? 1 : (d == 2 ? -1 : 0)), ay = py + (d == 1 ? 1 : (d == 3 ? -1 : 0));
    if (kk == 4) put(ax, ay, pz + 1);
    if (kk == 5) put(ax, ay, pz - 1);
    if (kk == 1 || kk >= 3) put(ax, ay, pz);
    if (kk == 2) put(px, py, pz + 1);
    c = p;
  }
}

// One term of the loss: -(distance of the statistic to its zero-loss interval [lo, hi]) * weight, rounded to double before it
// is added (no fused multiply-add): the Python rules bit for bit.
__device__ __forceinline__ double h3_target_term(double v, double lo, double hi, double weight) {
#pragma clang fp contract(off)
  const double d = v < lo ? lo - v : (v > hi ? v - hi : 0.0);
  return -d * weight;
}

__global__ __launch_bounds__(H3_THREADS) void mc3d_holey_kernel(const H3Args a) {
  __shared__ H3Lds L;
  const int tid = threadIdx.x;
  const bool dungeon = a.problem == H3_DUNGEON;
  const int nstat = dungeon ? 6 : 4, ntiles = dungeon ? 5 : 2;
  H3Dims dm;
  dm.BZ = a.Z + 2, dm.BY = a.Y + 2, dm.BX = a.X + 2;
  const int cells = dm.BZ * dm.BY * dm.BX, rows = dm.BZ * dm.BY, cols = dm.BY * dm.BX;
  const bool small = cells <= H3_SMALL_CELLS;
  uint8_t *slot = a.ws + (size_t)blockIdx.x * a.ws_stride;
  uint64_t *queue[2];
  H3State st[2];
  for (int s = 0; s < 2; s++) {
    uint8_t *base = slot + (size_t)s * (a.ws_stride / 2);
    queue[s] = (uint64_t *)base;
    if (small) {
      st[s].len = L.st16[s][0], st[s].jmp = L.st16[s][1], st[s].par = L.st16[s][2], st[s].ord = L.st16[s][3];
      st[s].kind = L.st8[s];
    } else {
      uint8_t *sb = base + (size_t)a.qcap * 8;
      const int64_t w = h3_align16(2 * (int64_t)cells);
      st[s].len = (uint16_t *)sb, st[s].jmp = (uint16_t *)(sb + w), st[s].par = (uint16_t *)(sb + 2 * w);
      st[s].ord = (uint16_t *)(sb + 3 * w), st[s].kind = sb + 4 * w;
    }
  }

  for (int lvl = blockIdx.x; lvl < a.n; lvl += gridDim.x) {
    __syncthreads();  // the previous level's LDS is done with
    const int32_t *hp = a.holes + (size_t)lvl * 6;
    int hz[2], hy[2], hx[2];
    bool holes_ok = true;
    for (int h = 0; h < 2; h++) {
      hz[h] = hp[h * 3 + 0], hy[h] = hp[h * 3 + 1], hx[h] = hp[h * 3 + 2];
      const bool face_x = (hx[h] == 0 || hx[h] == a.X + 1) && hy[h] >= 1 && hy[h] <= a.Y;
      const bool face_y = (hy[h] == 0 || hy[h] == a.Y + 1) && hx[h] >= 1 && hx[h] <= a.X;
      holes_ok = holes_ok && hz[h] >= 1 && hz[h] <= a.Z - 1 && (face_x || face_y);
    }
    // the bordered map
    const uint8_t *grid = a.grids + (size_t)lvl * a.Z * a.Y * a.X;
    bool bad = false;
    for (int i = tid; i < cells; i += H3_THREADS) {
      const int x = i % dm.BX, y = (i / dm.BX) % dm.BY, z = i / cols;
      uint8_t t = 1;
      if (x >= 1 && x <= a.X && y >= 1 && y <= a.Y && z >= 1 && z <= a.Z) {
        t = grid[((size_t)(z - 1) * a.Y + (y - 1)) * a.X + (x - 1)];
        if (t >= ntiles) {
          bad = true;
          t = 1;
        }
      }
      L.map[i] = t;
    }
    if (tid == 0) {
      L.seed = 0x7FFFFFFF, L.singles = 0, L.chest = 0x7FFFFFFF, L.n_chest = 0, L.n_enemy = 0, L.overflow = 0, L.far = -1;
      L.key_near = 0xFFFFFFFFu, L.key_far = 0;
      for (int s = 0; s < 2; s++) L.acc[s] = 0, L.pushed[s] = 0, L.rlen[s] = 0, L.legs[s] = 0, L.kept[s] = 0;
    }
    for (int i = tid; i < rows; i += H3_THREADS) L.ov[0][i] = 0, L.ov[1][i] = 0;
    for (int s = 0; s < 2; s++)
      for (int i = tid; i < cells; i += H3_THREADS) st[s].len[i] = 0;
    uint32_t err = __syncthreads_or(bad) ? H3_ERR_TILE : 0u;
    if (!holes_ok) err |= H3_ERR_HOLE;
    if (holes_ok && tid == 0)
      for (int h = 0; h < 2; h++) {
        L.map[h3_cell(dm, hx[h], hy[h], hz[h])] = 0;
        L.map[h3_cell(dm, hx[h], hy[h], hz[h] + 1)] = 0;
      }
    __syncthreads();

    int regions = 0;
    if (holes_ok) {
      // planes and counts
      int nc = 0, ne = 0, first_chest = 0x7FFFFFFF;
      for (int i = tid; i < cells; i += H3_THREADS) {
        const int t = L.map[i];
        if (t == 2) {
          nc++;
          first_chest = min(first_chest, i);
        }
        ne += t == 3 || t == 4;
      }
      if (nc) {
        atomicAdd(&L.n_chest, nc);
        atomicMin(&L.chest, first_chest);
      }
      if (ne) atomicAdd(&L.n_enemy, ne);
      for (int i = tid; i < cols; i += H3_THREADS) {
        uint32_t c = 0;
        for (int z = 0; z < dm.BZ; z++) c |= (uint32_t)(L.map[z * cols + i] != 1) << z;
        L.col[i] = c;
      }
      for (int r = tid; r < rows; r += H3_THREADS) {
        uint32_t m = 0;
        for (int x = 0; x < dm.BX; x++) m |= (uint32_t)(L.map[r * dm.BX + x] == 0) << x;
        L.air[r] = m;
      }
      __syncthreads();
      // AIR cells without an AIR neighbour: regions of one cell
      uint32_t keep[3] = {0, 0, 0};
      int singles = 0;
      for (int k = 0, r = tid; r < rows; r += H3_THREADS, k++) {
        const int z = r / dm.BY, y = r % dm.BY;
        const uint32_t m = L.air[r];
        uint32_t nb = (m << 1) | (m >> 1);
        if (y > 0) nb |= L.air[r - 1];
        if (y + 1 < dm.BY) nb |= L.air[r + 1];
        if (z > 0) nb |= L.air[r - dm.BY];
        if (z + 1 < dm.BZ) nb |= L.air[r + dm.BY];
        singles += __popc(m & ~nb);
        keep[k] = m & nb;
      }
      if (singles) atomicAdd(&L.singles, singles);
      __syncthreads();
      for (int k = 0, r = tid; r < rows; r += H3_THREADS, k++) L.air[r] = keep[k];  // from here: the AIR not yet counted
      __syncthreads();
      regions = L.singles;
      for (int guard = 0; guard < cells; guard++) {
        for (int r = tid; r < rows; r += H3_THREADS)
          if (L.air[r]) {
            atomicMin(&L.seed, r);
            break;
          }
        __syncthreads();
        const int seed = L.seed;
        if (seed == 0x7FFFFFFF) break;
        for (int r = tid; r < rows; r += H3_THREADS) {
          const uint32_t m = L.air[r];
          L.cur[0][r] = r == seed ? m & (0u - m) : 0u;
        }
        __syncthreads();
        if (tid == 0) L.seed = 0x7FFFFFFF;
        int b = 0;
        for (int sweep = 0; sweep < cells; sweep++, b ^= 1) {
          bool grew = false;
          for (int r = tid; r < rows; r += H3_THREADS) {
            const int z = r / dm.BY, y = r % dm.BY;
            const uint32_t m = L.air[r], old = L.cur[b][r];
            uint32_t f = old;
            if (y > 0) f |= L.cur[b][r - 1];
            if (y + 1 < dm.BY) f |= L.cur[b][r + 1];
            if (z > 0) f |= L.cur[b][r - dm.BY];
            if (z + 1 < dm.BZ) f |= L.cur[b][r + dm.BY];
            f &= m;
            for (int i = 0; i < H3_B; i++) {  // along x until the runs are full
              const uint32_t g = (f | (f << 1) | (f >> 1)) & m;
              if (g == f) break;
              f = g;
            }
            grew = grew || f != old;
            L.cur[b ^ 1][r] = f;
          }
          if (!__syncthreads_or(grew)) break;
        }
        for (int r = tid; r < rows; r += H3_THREADS) L.air[r] &= ~L.cur[b][r];  // cur[b] == cur[b ^ 1] after a still sweep
        regions++;
        __syncthreads();
      }
    }

    // the searches
    const int n_chest = L.n_chest, n_enemy = L.n_enemy, chest = L.chest;
    const int entrance = h3_cell(dm, hx[0], hy[0], hz[0]), exitc = h3_cell(dm, hx[1], hy[1], hz[1]);
    const bool run0 = holes_ok && (!dungeon || n_chest > 0 || n_enemy > 0), run1 = holes_ok && dungeon && n_chest > 0;
    if (tid == 0 && run0) {
      int acc, pushed;
      bool ovf;
      h3_search(L, dm, st[0], queue[0], (uint32_t)a.qcap - 1u, entrance, acc, pushed, ovf);
      L.acc[0] = acc, L.pushed[0] = pushed;
      if (ovf) atomicOr(&L.overflow, 1);
    }
    if (tid == 64 && run1) {
      int acc, pushed;
      bool ovf;
      h3_search(L, dm, st[1], queue[1], (uint32_t)a.qcap - 1u, chest, acc, pushed, ovf);
      L.acc[1] = acc, L.pushed[1] = pushed;
      if (ovf) atomicOr(&L.overflow, 1);
    }
    __threadfence_block();
    __syncthreads();
    const bool overflow = L.overflow != 0;
    if (overflow) err |= H3_ERR_QUEUE;
    const bool answer = holes_ok && !overflow;

    // the nearest enemy (SKULL before PUMPKIN, each in cell order, strict <) or the maze's first longest path
    if (answer && run0) {
      if (dungeon) {
        uint32_t key = 0xFFFFFFFFu;
        for (int i = tid; i < cells; i += H3_THREADS) {
          const int t = L.map[i], l = st[0].len[i];
          if ((t == 3 || t == 4) && l > 0) key = min(key, ((uint32_t)l << 14) | ((uint32_t)(t == 4) << 13) | (uint32_t)i);
        }
        if (key != 0xFFFFFFFFu) atomicMin(&L.key_near, key);
      } else {
        uint32_t key = 0;
        for (int i = tid; i < cells; i += H3_THREADS) {
          const int l = st[0].len[i];
          if (l > 0) key = max(key, ((uint32_t)l << 13) | (8191u - (uint32_t)st[0].ord[i]));
        }
        if (key) atomicMax(&L.key_far, key);
      }
    }
    __syncthreads();
    int near_cell = -1;
    if (answer && dungeon && L.key_near != 0xFFFFFFFFu) near_cell = (int)(L.key_near & 0x1FFFu);
    if (answer && !dungeon && run0) {
      const uint32_t key = L.key_far;
      const int bl = (int)(key >> 13), bo = (int)(8191u - (key & 0x1FFFu));
      for (int i = tid; i < cells; i += H3_THREADS)
        if (st[0].len[i] == bl && st[0].ord[i] == bo) L.far = i;
    }
    __syncthreads();
    const int far = L.far;

    // the routes: thread 0 the main one, thread 64 the second
    if (answer && tid == 0) {
      int16_t *co = (a.coords && a.route_cap > 0) ? a.coords + (size_t)lvl * a.route_cap * 3 : nullptr;
      if (dungeon) {
        if (n_chest > 0) {
          const int lc = st[0].len[chest], ld = st[1].len[exitc];
          if (lc > 0) h3_walk(dm, st[0], chest, 0, co, a.route_cap, L.ov[0]);
          if (ld > 0) h3_walk(dm, st[1], exitc, lc, co, a.route_cap, L.ov[0]);
          L.legs[0] = lc, L.legs[1] = ld, L.rlen[0] = lc + ld;
        }
      } else {
        const int l = st[0].len[exitc];
        if (l > 0) h3_walk(dm, st[0], exitc, 0, co, a.route_cap, L.ov[0]);
        L.rlen[0] = l;
      }
    }
    if (answer && tid == 64) {
      int16_t *co = (a.coords2 && a.route_cap > 0) ? a.coords2 + (size_t)lvl * a.route_cap * 3 : nullptr;
      const int target = dungeon ? near_cell : far;
      if (target >= 0) {
        h3_walk(dm, st[0], target, 0, co, a.route_cap, L.ov[1]);
        L.rlen[1] = st[0].len[target];
      }
    }
    __threadfence_block();
    __syncthreads();

    // remove_stacked_path_tiles of both routes, and the overlays
    for (int o = 0; o < 2; o++) {
      uint8_t *out = o == 0 ? a.overlay : a.overlay2;
      int kept = 0;
      for (int r = tid; r < rows; r += H3_THREADS) {
        const uint32_t m = L.ov[o][r] & ~(r >= dm.BY ? L.ov[o][r - dm.BY] : 0u);
        kept += __popc(m);
        if (out)
          for (int x = 0; x < dm.BX; x++) out[(size_t)lvl * cells + (size_t)r * dm.BX + x] = (uint8_t)((m >> x) & 1u);
      }
      if (kept) atomicAdd(&L.kept[o], kept);
    }
    __syncthreads();
    const int rlen0 = L.rlen[0], rlen1 = L.rlen[1];
    if (a.route_cap > 0) {
      if (a.coords)
        for (int i = rlen0 * 3 + tid; i < a.route_cap * 3; i += H3_THREADS) a.coords[(size_t)lvl * a.route_cap * 3 + i] = -1;
      if (a.coords2)
        for (int i = rlen1 * 3 + tid; i < a.route_cap * 3; i += H3_THREADS) a.coords2[(size_t)lvl * a.route_cap * 3 + i] = -1;
    }
    if (tid == 0) {
      int32_t s[H3_MAX_STATS] = {-1, -1, -1, -1, -1, -1};
      if (answer) {
        if (dungeon) {
          s[0] = regions, s[1] = L.rlen[0], s[2] = n_chest, s[3] = n_enemy;
          s[4] = near_cell >= 0 ? (int)st[0].len[near_cell] : 0;
          s[5] = 0;
          if (n_chest > 0) s[5] = (L.legs[0] > 0 ? (int)st[0].jmp[chest] : 0) + (L.legs[1] > 0 ? (int)st[1].jmp[exitc] : 0);
        } else {
          s[0] = regions, s[1] = L.kept[1];
          s[2] = rlen0 > 0 ? rlen0 : -1;
          s[3] = rlen0 > 0 ? (int)st[0].jmp[exitc] : 0;
        }
      }
      for (int k = 0; k < nstat; k++) a.stats[(size_t)lvl * nstat + k] = s[k];
      if (a.loss) {
        double loss = 0.0;
        for (int k = 0; k < nstat; k++) loss = loss + h3_target_term((double)s[k], a.trg_lo[k], a.trg_hi[k], a.weight[k]);
        a.loss[lvl] = answer ? loss : -__builtin_huge_val();
      }
      if (a.play) {
        int32_t *p = a.play + (size_t)lvl * H3_PLAY;
        for (int k = 0; k < H3_PLAY; k++) p[k] = 0;
        for (int k = 5; k < 11; k++) p[k] = -1;
        if (answer) {
          p[0] = (run0 ? 1 : 0) | (run1 ? 2 : 0);
          p[1] = L.acc[0], p[2] = L.pushed[0], p[3] = L.acc[1], p[4] = L.pushed[1];
          const int c5 = dungeon ? (n_chest > 0 ? chest : -1) : far, c8 = dungeon ? near_cell : -1;
          if (c5 >= 0) p[5] = c5 % dm.BX, p[6] = (c5 / dm.BX) % dm.BY, p[7] = c5 / cols;
          if (c8 >= 0) p[8] = c8 % dm.BX, p[9] = (c8 / dm.BX) % dm.BY, p[10] = c8 / cols;
        }
      }
      if (a.route_len) a.route_len[lvl] = rlen0;
      if (a.route2_len) a.route2_len[lvl] = rlen1;
      if (a.leg_len) a.leg_len[(size_t)lvl * 2] = L.legs[0], a.leg_len[(size_t)lvl * 2 + 1] = L.legs[1];
      if (a.error) a.error[lvl] = err;
    }
  }
}

#endif  // PCGRL_H3_KERNEL

}  // namespace pcgrl
