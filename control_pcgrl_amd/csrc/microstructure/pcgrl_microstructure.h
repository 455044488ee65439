// microstructure/pcgrl_microstructure.h -- microstructure levels on the device (include/pcgrl_amd_microstructure.h): what
// MicroStructureProblem.get_stats computes for a two-phase map -- helper.py:278-318 calc_tortuosity over the empty cells -- the
// loss ControlWrapper.get_loss would derive from it, the per-region record behind both statistics, and the level measures and
// the bit-plane image of such maps.  DESIGN.md section 30 has the rules with every quirk; tests/microstructure_rules.py is the
// same in plain Python.
//
// microstructure_kernel: one 64-lane wave per map, lane = row, a row of the map one uint64_t mask of its empty cells (bit c =
// column c), 1..64 rows x 1..64 columns.  The searches are the level-synchronous sweeps of pcgrl_kernels2d.h, included as they
// are (Grp<64>, expand, sweep, first_rowmajor): the reference's first-in first-out flood gives breadth-first distances, so a
// sweep's number of levels is np.max of the flood's map and the first row-major cell of its last level is np.argmax.
//   map       the bytes are staged in LDS by meas_wave_stage (16-byte loads at any alignment); per 64-cell chunk one ballot of
//             `id == 0` is a word of the map's row-major bit string, kept by the lane of that number; a row's mask is cut out of
//             the two words it may span.  An id above 1 reads as solid and raises error bit 0.
//   regions   one-cell regions take no sweep: iso = pass & ~expand(pass).  The others are peeled off in row-major order of
//             their first cell: a sweep from it inside what is left, the first row-major cell of its last level (the far cell),
//             a second sweep from the far cell inside the region just visited: its levels are the region's d.  path-length is
//             the largest d.  l2 = sqrt(dx * dx + dy * dy) from the first cell to the far cell (0 replaced by 1), tort = d / l2:
//             one correctly rounded square root and one division in double.
//   mean      np.mean takes the values in visit order, the one-cell regions' zeros included, and adds them pairwise, so a
//             value's position matters: a swept region's index is the number of swept regions before it plus the one-cell
//             regions whose cell lies before its first cell.  The values go to vals[], zeroed first: at most ceil(H * W / 2)
//             = 2 048 doubles (components are pairwise non-adjacent).  Lane 0 then adds them in numpy's order -- below 8 in
//             sequence; up to 128 through eight interleaved accumulators combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then
//             the remainder; above 128 split in halves, the first rounded down to a multiple of 8 -- with the split tree walked
//             through a small explicit stack, and divides once by the count.
//   record    with region_cap > 0: a swept region writes its entry when it is found (its tort is above 0, which marks its
//             slot in vals[]); the slots left are the one-cell regions in row-major order, filled in afterwards; entries past
//             the last region are -1 (tort 0).  Every entry is written once.
// 16 KiB of LDS for vals[] (the staged bytes lie in the same space: they are dead before it is zeroed) and 256 B for the stack;
// no workspace in global memory.
//
// ms_measures_kernel: one wave per map; the per-map body is meas_wave_map<2, 1, 4096> of measures/pcgrl_measures_wave.h, the
// engine's binary form (ids masked to 1 bit).  The pairwise step is measures/pcgrl_measures.h's, launched as it is.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../measures/pcgrl_measures_wave.h"  // MeasWaveArgs, meas_wave_stage, meas_wave_map

namespace pcgrl {

constexpr int MS_STATS = 2;  // path-length, tortuosity
constexpr int MS_MAX_H = 64, MS_MAX_W = 64, MS_MAX_CELLS = MS_MAX_H * MS_MAX_W;
constexpr int MS_MAX_REGIONS = MS_MAX_CELLS / 2;  // 2 048: the 64 x 64 checkerboard
constexpr int MS_REC_FIELDS = 5;                  // start row, start column, far row, far column, d
constexpr int MS_MEAS_TILES = 2, MS_MEAS_PLANES = 1;
constexpr int MS_STACK = 16;  // the split tree of 2 048 values is 4 deep: at most 11 pending items, 6 values

struct MsArgs {
  int32_t h, w, n;
  const uint8_t *grids;  // uint8 [n][h][w] at any alignment
  int32_t region_cap;
  double *stats;         // [n][2]
  double *loss;          // [n] or null
  int32_t *regions;      // [n] or null
  int16_t *region_rec;   // [n][region_cap][5] or null
  double *region_tort;   // [n][region_cap] or null
  uint32_t *error;       // [n] or null
  int32_t has_trg[MS_STATS];
  double weight[MS_STATS], trg_lo[MS_STATS], trg_hi[MS_STATS];
};

hipError_t launch_microstructure(const MsArgs &a, hipStream_t s);
hipError_t launch_ms_measures(const MeasWaveArgs &a, hipStream_t s);

}  // namespace pcgrl

#ifdef PCGRL_MS_KERNEL  // (microstructure/pcgrl_k_microstructure.hip has it)
#include "../pcgrl_kernels2d.h"  // Grp, expand, sweep, first_rowmajor -- unedited

namespace pcgrl {

// One term of the loss: -(distance of the statistic to its zero-loss interval [lo, hi]) * weight, rounded to double before it
// is added (no fused multiply-add): the Python rules bit for bit.
__device__ __forceinline__ double ms_target_term(double v, double lo, double hi, double weight) {
#pragma clang fp contract(off)
  const double d = v < lo ? lo - v : (v > hi ? v - hi : 0.0);
  return -d * weight;
}

// numpy's pairwise sum of at most 128 values (one lane)
__device__ __forceinline__ double ms_sum_block(const double *v, int n) {
#pragma clang fp contract(off)
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; i++) res = res + v[i];
    return res;
  }
  double r0 = v[0], r1 = v[1], r2 = v[2], r3 = v[3], r4 = v[4], r5 = v[5], r6 = v[6], r7 = v[7];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 = r0 + v[i];
    r1 = r1 + v[i + 1];
    r2 = r2 + v[i + 2];
    r3 = r3 + v[i + 3];
    r4 = r4 + v[i + 4];
    r5 = r5 + v[i + 5];
    r6 = r6 + v[i + 6];
    r7 = r7 + v[i + 7];
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; i++) res = res + v[i];
  return res;
}

// numpy's pairwise sum of v[0 .. n), 1 <= n <= MS_MAX_REGIONS (one lane).  The recursion sum(v, n) = sum(v, n2) +
// sum(v + n2, n - n2) is walked with two stacks: pending items (a segment to add up, or "add the two values on top") and values.
__device__ inline double ms_sum(const double *v, int n, int32_t (*todo)[2], double *val) {
#pragma clang fp contract(off)
  int nt = 0, nv = 0;
  todo[nt][0] = 0;
  todo[nt++][1] = n;
  while (nt > 0) {
    nt--;
    const int off = todo[nt][0], len = todo[nt][1];
    if (len == 0) {  // add the two values on top
      nv--;
      val[nv - 1] = val[nv - 1] + val[nv];
    } else if (len <= 128) {
      val[nv++] = ms_sum_block(v + off, len);
    } else {
      int n2 = len / 2;
      n2 -= n2 % 8;
      todo[nt][0] = 0;
      todo[nt++][1] = 0;
      todo[nt][0] = off + n2;
      todo[nt++][1] = len - n2;
      todo[nt][0] = off;
      todo[nt++][1] = n2;
    }
  }
  return val[0];
}

__device__ __forceinline__ uint64_t ms_shfl64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// the column of the one bit that lane `src` (the same in every lane) holds in x
__device__ __forceinline__ int ms_col(const Grp<64> &g, uint64_t x, int src) {
  return (int)g.gbcast(x ? (uint32_t)ctz_m(x) : 0u, src);
}

__global__ __launch_bounds__(64) void microstructure_kernel(const MsArgs a) {
#pragma clang fp contract(off)
  // the staged map bytes (MS_MAX_CELLS + 32 of them) first, then the regions' values: the bytes are dead before vals is zeroed
  __shared__ __attribute__((aligned(16))) double vals[MS_MAX_REGIONS];
  __shared__ int32_t todo[MS_STACK][2];
  __shared__ double val[MS_STACK];
  const int e = blockIdx.x;
  if (e >= a.n) return;
  Grp<64> g;
  g.init();
  const int lane = g.lane, H = a.h, W = a.w, n = H * W, NW = (n + 63) >> 6;

  MeasWaveArgs st{};
  st.grids = a.grids;
  st.stride = n;
  st.h = H;
  st.w = W;
  const uint8_t *m = meas_wave_stage(st, e, (uint8_t *)vals);
  uint64_t word = 0, bad = 0;  // lane k: bits 64 k .. 64 k + 63 of the row-major string of empty cells
  for (int ch = 0; ch < NW; ch++) {
    const int i = ch * 64 + lane;
    const bool ok = i < n;
    const uint8_t id = m[ok ? i : 0];
    const uint64_t b = __ballot(ok && id == 0);
    bad |= __ballot(ok && id > 1);
    if (lane == ch) word = b;
  }
  const int first = lane * W, k = first >> 6, sh = first & 63;  // first <= 63 * 64, so k <= 63
  const uint64_t lo = ms_shfl64(word, k), hi = ms_shfl64(word, k < 63 ? k + 1 : 63);
  const uint64_t cut = sh ? ((lo >> sh) | (hi << (64 - sh))) : lo;
  const uint64_t pass = lane < H ? (cut & (W == 64 ? ~0ull : ((1ull << W) - 1ull))) : 0ull;
  __syncthreads();
  const int vcap = (n + 1) >> 1;
  for (int i = lane; i < vcap; i += 64) vals[i] = 0.0;
  __syncthreads();

  const int cap = a.region_cap;
  int16_t *rec = a.region_rec ? a.region_rec + (size_t)e * cap * MS_REC_FIELDS : nullptr;
  const uint64_t iso = pass & ~expand(g, pass);
  const int n_iso = (int)g.gsum((uint32_t)popc_m(iso));
  uint64_t remaining = pass & ~iso;
  int swept = 0, path = 0;
  while (true) {
    const uint64_t gb = __ballot(remaining != 0);
    if (gb == 0) break;
    const int sr = __builtin_ctzll(gb);
    const uint64_t seed = lane == sr ? (remaining & (0ull - remaining)) : 0ull;
    const int sc = ms_col(g, seed, sr);
    int depth, d;
    uint64_t last, vis, last2, vis2;
    sweep(g, seed, remaining, depth, last, vis);
    uint64_t far = first_rowmajor(g, last);
    uint64_t fb = __ballot(far != 0);
    if (fb == 0) {  // (a region that is not a single cell always reaches level 1)
      far = seed;
      fb = 1ull << sr;
    }
    const int fr = __builtin_ctzll(fb);
    const int fc = ms_col(g, far, fr);
    sweep(g, far, vis, d, last2, vis2);
    remaining &= ~vis;
    path = d > path ? d : path;
    const int dx = sc - fc, dy = sr - fr;
    double l2 = sqrt((double)(dx * dx + dy * dy));
    if (!(l2 > 0.0)) l2 = 1.0;
    const double tort = (double)d / l2;
    // the one-cell regions visited before this one: those in the rows above, and those left of the first cell in its row
    const uint32_t before = lane < sr ? (uint32_t)popc_m(iso) : (lane == sr ? (uint32_t)popc_m((uint64_t)(iso & (seed - 1ull))) : 0u);
    const int idx = swept + (int)g.gsum(before);
    if (lane == 0 && idx < vcap) {
      vals[idx] = tort;
      if (rec && idx < cap) {
        int16_t *r = rec + idx * MS_REC_FIELDS;
        r[0] = (int16_t)sr;
        r[1] = (int16_t)sc;
        r[2] = (int16_t)fr;
        r[3] = (int16_t)fc;
        r[4] = (int16_t)d;
      }
    }
    swept++;
  }
  __syncthreads();
  const int total = swept + n_iso;  // <= vcap

  if (rec) {
    const int seen = total < vcap ? total : vcap;
    const int lim = seen < cap ? seen : cap;
    uint64_t left = iso;
    for (int j = 0; j < lim; j++) {
      if (__ballot(vals[j] != 0.0) != 0) continue;  // a swept region's slot
      const uint64_t gb = __ballot(left != 0);
      if (gb == 0) break;
      const int r = __builtin_ctzll(gb);
      const uint64_t bit = lane == r ? (left & (0ull - left)) : 0ull;
      const int c = ms_col(g, bit, r);
      left ^= bit;
      if (lane == 0) {
        int16_t *o = rec + j * MS_REC_FIELDS;
        o[0] = (int16_t)r;
        o[1] = (int16_t)c;
        o[2] = (int16_t)r;
        o[3] = (int16_t)c;
        o[4] = 0;
      }
    }
    for (int j = lim * MS_REC_FIELDS + lane; j < cap * MS_REC_FIELDS; j += 64) rec[j] = (int16_t)-1;
  }
  if (a.region_tort) {
    double *o = a.region_tort + (size_t)e * cap;
    for (int j = lane; j < cap; j += 64) o[j] = (j < total && j < vcap) ? vals[j] : 0.0;
  }
  if (lane != 0) return;
  double st2[MS_STATS];
  st2[0] = (double)path;
  st2[1] = total > 0 ? ms_sum(vals, total < vcap ? total : vcap, todo, val) / (double)total : 0.0;
  a.stats[(size_t)e * MS_STATS] = st2[0];
  a.stats[(size_t)e * MS_STATS + 1] = st2[1];
  if (a.loss) {
    double loss = 0.0;
#pragma unroll
    for (int s = 0; s < MS_STATS; s++)
      if (a.has_trg[s]) loss = loss + ms_target_term(st2[s], a.trg_lo[s], a.trg_hi[s], a.weight[s]);
    a.loss[e] = loss;
  }
  if (a.regions) a.regions[e] = total;
  if (a.error) a.error[e] = bad ? 1u : 0u;
}

__global__ __launch_bounds__(64) void ms_measures_kernel(const MeasWaveArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t cells[MS_MAX_CELLS + 32];
  const int e = blockIdx.x;
  if (e >= a.n) return;
  meas_wave_map<MS_MEAS_TILES, MS_MEAS_PLANES, MS_MAX_CELLS>(a, e, cells);
}

}  // namespace pcgrl
#endif  // PCGRL_MS_KERNEL
