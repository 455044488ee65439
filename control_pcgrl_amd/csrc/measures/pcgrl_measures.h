// measures/pcgrl_measures.h -- level measures and pairwise Hamming diversity of 2-D maps on the device
// (include/pcgrl_amd_measures.h): the integers behind the reference's behaviour characteristics (evo/evolve.py:423-592) and
// behind div_calc (rl/evaluate_ctrl.py:42-48) / diversity_bonus (evo/evolve.py:1236-1244).
//
// The rules (m[H][W] tile ids masked to P = ceil(log2 T) bits, n = H * W):
//   counts[t]   cells with tile t, t < T (get_counts, get_emptiness, get_entropy)
//   match[0]    "horizontal": cells (r, c), r < H / 2, with m[r][c] == m[H - 1 - r][c] (get_hor_sym; the middle row of an odd H
//               is left out)
//   match[1]    "vertical": cells (r, c), c < W / 2, with m[r][c] == m[r][W - 1 - c] (get_ver_sym)
//   match[2]    co-occurance: over all cells the four np.roll neighbours that hold the same tile -- the rolls WRAP, so with
//               H == 1 a cell is its own vertical neighbour (twice) and with H == 2 both vertical rolls meet the same cell
//   entropy     e = 0.0; for t = 0 .. T - 1 in order: if counts[t] != 0: e -= tab[counts[t]]; e / tab[n + 1], where the caller's
//               table holds tab[c] = (c / n) * ln(c / n) and tab[n + 1] = -(1 / T) * ln(1 / T) * T (get_entropy's max_val)
//   forms       the float64 forms of the integers, each one or two correctly rounded double operations in the reference's
//               order: counts[0] / n, match[0] / (W * H / 2), match[1] / (W * H / 2), (vertical + horizontal) / 2.0,
//               match[2] / (n * 4), then counts[t] / n for every t; per group S / (K (K - 1)) / n and 10 * (S / (K K - 1)) / n
//               (diversity_scores_kernel, after the sums are complete).  No fast-math, no contraction: bit for bit numpy's.
//   d(a, b)     cells whose tiles differ = sum over 64-cell words w of popcount(OR_p (a[p][w] ^ b[p][w]))
//   per group of K consecutive maps: S = sum of d over all ordered pairs; nearest[i] = min_{k != i} d(i, k) and the lowest
//   such k; optionally the full K x K matrix
//
// measures_kernel<T, P>: one 64-lane wave per map, any shape up to 64 x 64; (T, P) = (2, 1) binary, (5, 3) sokoban, (8, 3)
// zelda.  The map's bytes are staged in LDS with 16-byte loads (caller maps: meas_wave_stage of measures/pcgrl_measures_wave.h)
// or expanded here from the engine's bit-planes; then meas_wave_body<T, P> of that header: per 64-cell chunk a lane holds one
// cell, __ballot((id >> p) & 1) IS word p of the chunk in the bit-plane image the pairwise kernel reads ([map][P][NW] uint64,
// NW = ceil(n / 64), tail lanes contribute 0), and the counts and matches are popcounts of ballots; the partner cells come
// from LDS.  4 112 B of LDS.
//
// diversity_kernel: one 64-lane workgroup owns 64 row maps of one group, one per lane, and walks a range of the group's maps
// ("columns") in tiles of DIV_TC = 16; the columns of a group are cut into `splits` ranges so that a call fills the device
// (div_splits: about DIV_TARGET_WGS workgroups), whatever K and the number of groups are.  A column tile sits in LDS in the image's own layout (one contiguous copy, <= 24 KB) and is read at
// wave-uniform addresses (broadcast reads); the row map's words sit in registers, DIV_WC = 4 words x P planes at a time
// (a 64 x 64 three-plane map has 192 words; the chunk keeps 24 VGPRs), with 16 running distances per lane.  The whole
// square is computed (no cross-lane minimum for the columns); each lane keeps the nearest distance / index of its column
// range (ascending columns, strict <) and its row sum in 64 bits.  The ranges meet in memory: the group sum is one wave
// reduction and one 64-bit vector atomic add per workgroup onto a word measures_kernel zeroed, the nearest map one 64-bit
// vector atomic min per lane of the key (distance << 32 | index) onto a word measures_kernel set to all ones -- the least
// key is the least distance and among those the lowest index; integers, so both are deterministic in any order.
// diversity_finish_kernel unpacks the keys and makes the two scores.  The matrix is written through its symmetry,
// pairwise[j][i] = d(i, j), so that a wave's store is contiguous.
#pragma once
#include <hip/hip_runtime.h>

#include "../pcgrl_common.h"
#include "pcgrl_measures_wave.h"  // MEAS_FORMS, MeasWaveArgs, the per-map wave body

namespace pcgrl {

constexpr int MEAS_MAX_CELLS = 64 * 64;
constexpr int DIV_TC = 16;  // column maps per LDS tile = running distances per lane
constexpr int DIV_WC = 4;   // words per plane of the row map held in registers at a time
constexpr int DIV_TARGET_WGS = 2048;  // one-wave workgroups a call aims for: 2 per SIMD of 256 CUs

struct DivArgs {
  const uint64_t *pack;  // [n][P][NW]
  int32_t n, K, P, NW;
  int32_t splits;           // column ranges per group, each tiles_per_split tiles of DIV_TC columns (none empty)
  int32_t tiles_per_split;
  unsigned long long *sum;  // [n / K]
  unsigned long long *near_key;  // [n] (distance << 32 | index within the group)
  int32_t *pairwise;        // [n / K][K][K] or null
};

// the column ranges of a group: enough of them for about DIV_TARGET_WGS workgroups, whole tiles, none empty
inline void div_splits(int n, int K, int &splits, int &tiles_per_split) {
  const int col_tiles = (K + DIV_TC - 1) / DIV_TC, row_wgs = (n / K) * ((K + 63) / 64);
  int want = (DIV_TARGET_WGS + row_wgs - 1) / row_wgs;
  want = want < 1 ? 1 : (want > col_tiles ? col_tiles : want);
  tiles_per_split = (col_tiles + want - 1) / want;
  splits = (col_tiles + tiles_per_split - 1) / tiles_per_split;
}

inline int meas_planes(int n_tiles) {
  int p = 0;
  while ((1 << p) < n_tiles) p++;
  return p;
}

// a.grids null: the engine's own maps (p.planes); a.h, a.w the engine's map shape, T = p.n_tiles one of 2, 5, 8
hipError_t launch_measures(const Params &p, const MeasWaveArgs &a, hipStream_t s);
hipError_t launch_diversity(const DivArgs &a, hipStream_t s);
// nearest / nearest_idx from the keys (each may be null); scores[g] = (div_calc, diversity_bonus) of sum[g] (may be null)
hipError_t launch_diversity_finish(const DivArgs &a, int32_t n_cells, int32_t *nearest, int32_t *nearest_idx, double *scores,
                                   hipStream_t s);

}  // namespace pcgrl

#ifdef PCGRL_KERNEL_TU
#include "../pcgrl_kernels2d.h"  // ROW_WORDS: the plane layout of the engine's maps

namespace pcgrl {

template <int T, int P>
__global__ __launch_bounds__(64) void measures_kernel(Params p, MeasWaveArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t cells[MEAS_MAX_CELLS + 16];
  const int lane = threadIdx.x, e = blockIdx.x;
  const uint8_t *m = cells;
  if (a.grids != nullptr) {
    m = meas_wave_stage(a, e, cells);
  } else {
    const int H = a.h, W = a.w, n = H * W;
    const int dr = 64 / W, dc = 64 - dr * W;  // 64 cells further on: dr rows and dc columns
    int r = lane / W, c = lane - r * W;
    for (int i = lane; i < n; i += 64) {
      int id = 0;
      if (W > 32) {
        const uint64_t *pl = (const uint64_t *)p.planes + (size_t)e * ROW_WORDS * H;
#pragma unroll
        for (int k = 0; k < P; k++) id |= (int)((pl[k * H + r] >> c) & 1u) << k;
      } else {
        const uint32_t *pl = (const uint32_t *)p.planes + (size_t)e * ROW_WORDS * H;
#pragma unroll
        for (int k = 0; k < P; k++) id |= (int)((pl[k * H + r] >> c) & 1u) << k;
      }
      cells[i] = (uint8_t)id;
      c += dc;
      r += dr;
      if (c >= W) {
        c -= W;
        r++;
      }
    }
    __syncthreads();
  }
  meas_wave_body<T, P>(a, e, m);
}

template <int P>
__global__ __launch_bounds__(64) void diversity_kernel(DivArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint64_t col[];  // [DIV_TC][P][NW]
  const int lane = threadIdx.x;
  const int K = a.K, NW = a.NW;
  const int per_group = ((K + 63) / 64) * a.splits;
  const int g = blockIdx.x / per_group, rem = blockIdx.x - g * per_group;
  const int i = (rem / a.splits) * 64 + lane;
  const int j_lo = (rem % a.splits) * a.tiles_per_split * DIV_TC;
  const int j_hi = j_lo + a.tiles_per_split * DIV_TC < K ? j_lo + a.tiles_per_split * DIV_TC : K;
  const bool rowok = i < K;
  const int mw = P * NW;  // words per map
  const uint64_t *grp = a.pack + (size_t)g * K * mw;
  const uint64_t *row = grp + (size_t)(rowok ? i : K - 1) * mw;
  const bool single = NW <= DIV_WC;  // the whole row map fits the register chunk: loaded once
  uint64_t ar[P][DIV_WC];
  if (single) {
#pragma unroll
    for (int k = 0; k < P; k++)
#pragma unroll
      for (int w = 0; w < DIV_WC; w++) ar[k][w] = w < NW ? row[k * NW + w] : 0ull;
  }
  int best = 0x7fffffff, besti = 0;
  long long rsum = 0;
  for (int j0 = j_lo; j0 < j_hi; j0 += DIV_TC) {
    const int nc = j_hi - j0 < DIV_TC ? j_hi - j0 : DIV_TC;
    __syncthreads();  // the previous tile has been read
    const uint64_t *src = grp + (size_t)j0 * mw;
    for (int x = lane; x < nc * mw; x += 64) col[x] = src[x];
    __syncthreads();
    int acc[DIV_TC];
#pragma unroll
    for (int j = 0; j < DIV_TC; j++) acc[j] = 0;
    for (int c0 = 0; c0 < NW; c0 += DIV_WC) {
      if (!single) {
#pragma unroll
        for (int k = 0; k < P; k++)
#pragma unroll
          for (int w = 0; w < DIV_WC; w++) ar[k][w] = c0 + w < NW ? row[k * NW + c0 + w] : 0ull;
      }
#pragma unroll
      for (int j = 0; j < DIV_TC; j++) {
        if (j < nc) {  // (wave-uniform)
          const uint64_t *cj = col + j * mw + c0;
#pragma unroll
          for (int w = 0; w < DIV_WC; w++) {
            if (c0 + w < NW) {  // (wave-uniform)
              uint64_t x = ar[0][w] ^ cj[w];
#pragma unroll
              for (int k = 1; k < P; k++) x |= ar[k][w] ^ cj[k * NW + w];
              acc[j] += __popcll(x);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < DIV_TC; j++) {
      if (j < nc) {
        const int jj = j0 + j, d = acc[j];
        rsum += d;  // (the diagonal adds 0)
        if (jj != i && d < best) {
          best = d;
          besti = jj;
        }
        if (a.pairwise != nullptr && rowok) a.pairwise[((size_t)g * K + jj) * K + i] = d;
      }
    }
  }
  if (rowok) {
    if (best != 0x7fffffff) atomicMin(&a.near_key[(size_t)g * K + i], ((unsigned long long)best << 32) | (unsigned)besti);
  } else {
    rsum = 0;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) rsum += __shfl_xor(rsum, s, 64);
  if (lane == 0) atomicAdd(&a.sum[g], (unsigned long long)rsum);
}

__global__ __launch_bounds__(64) void diversity_finish_kernel(DivArgs a, int32_t n_cells, int32_t *nearest, int32_t *nearest_idx,
                                                              double *scores) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g < a.n) {
    const unsigned long long key = a.near_key[g];
    if (nearest != nullptr) nearest[g] = (int32_t)(key >> 32);
    if (nearest_idx != nullptr) nearest_idx[g] = (int32_t)(key & 0xffffffffull);
  }
  if (scores == nullptr || g >= a.n / a.K) return;
  const double S = (double)(long long)a.sum[g], k = (double)a.K, cells = (double)n_cells;
  scores[2 * g] = S / (k * (k - 1.0)) / cells;              // div_calc (evaluate_ctrl.py:42-48); K (K - 1) < 2^53: exact
  scores[2 * g + 1] = 10.0 * (S / (k * k - 1.0)) / cells;  // evolve.py:1236-1244: N * N - 1, then 10 * ... / (width * height)
}

}  // namespace pcgrl
#endif
