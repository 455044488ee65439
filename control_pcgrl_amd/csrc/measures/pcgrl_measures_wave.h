// measures/pcgrl_measures_wave.h -- the per-map wave body of every measure / pack kernel: one 64-lane wave computes, for one
// map of bytes, the quantities of measures/pcgrl_measures.h (its header comment states the rules and the order of the double
// operations; tests/measures_numpy.py is the same in numpy) and the map's words of the bit-plane image that diversity_kernel /
// diversity_finish_kernel read.  Written once as device function templates over
//   T     tile types (counted ids 0 .. T - 1),
//   P     bit planes of the image; ids are masked to P bits before anything else,
//   CAP   the most cells a map may have (a multiple of 64, at most 4 096: lane w keeps word w of each plane),
// and instantiated by the kernel of a problem: measures/pcgrl_measures.h (T, P = 2, 1 / 5, 3 / 8, 3; CAP = 4 096),
// smb/pcgrl_smb_measures.h (7, 3, 2 048), loderunner/pcgrl_loderunner_measures.h (8, 3, 512).  MeasWaveArgs is the one
// argument block of them all.
//
// All 64 lanes of the one-wave workgroup call these together for map e < a.n.
//   meas_wave_stage(a, e, cells)     the map's H * W bytes come from a.grids + e * a.stride at ANY alignment with 16-byte loads:
//             the aligned 16-byte blocks that hold the map's first and last byte are read whole (an aligned block that holds a
//             byte of the caller's buffer lies in the same page as that byte), into `cells`, at least CAP + 16 bytes of 16-byte
//             aligned LDS: at most (15 + CAP + 15) / 16 blocks = CAP + 16 bytes written.  Then the barrier; returns the map's
//             first byte in LDS, cells + off.  Two map sources, one code path:
//               caller maps   uint8 [n][H][W], stride = H * W;
//               padded rows   a 16-byte aligned base and stride = H * W rounded up to 16 (the committed maps of an smb env
//                             handle): off = 0 and the loads are the row's stride / 16 blocks, all of them the handle's own.
//             A stride that is neither reads blocks that belong to no map: a caller of this header passes one of the two.
//   meas_wave_body<T, P>(a, e, m)    m: the map's bytes in LDS, written before a barrier.
//     chunks  per 64-cell chunk a lane holds one cell; __ballot((id >> p) & 1) IS word p of the chunk in the image
//             ([map][P][NW] uint64; the lanes past the map's last cell contribute 0), the counts and the matches are popcounts
//             of ballots, and the partner cells (mirror row, mirror column, the four wrapped neighbours) come from LDS, which
//             holds the whole map, so nothing depends on where a chunk ends.  A lane's cell moves on by 64 cells per chunk:
//             64 / W rows and the rest in columns with one carry (W > 64: no row, 64 columns).
//     outputs lane w < NW writes word w of each plane; lane 0 writes the integers, the float64 forms, the entropy through the
//             caller's table, and -- with the image -- zeroes its group's sum and sets the map's nearest key to all ones for
//             diversity_kernel's atomics.  Every output pointer may be null.
//   meas_wave_map<T, P, CAP>(a, e, cells)   the two in sequence.
// Shapes: 1 <= H, 1 <= W, H * W <= CAP; the edge cases fall out of the rules as written:
//   H == 1 / W == 1   the wrapped neighbour along that axis is the cell itself, twice (2 matches per cell), and H / 2 == 0 /
//                     W / 2 == 0 leaves no symmetry pairs along it;
//   H == 2 / W == 2   both rolls along that axis meet the same cell;
//   odd H / W         the middle row / column is in no symmetry pair; the divisor W * H / 2 is a float division.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcgrl {

constexpr int MEAS_FORMS = 5;  // emptiness, symmetry-horizontal, symmetry-vertical, symmetry, co-occurance; then T fractions

struct MeasWaveArgs {
  const uint8_t *grids;  // map e starts at grids + e * stride (above); null only for measures_kernel: the engine's planes
  int32_t stride;        // bytes from one map's first byte to the next
  int32_t h, w, n, NW;   // NW = ceil(H * W / 64)
  int32_t *counts;       // [n][T], or null
  int32_t *match;        // [n][3], or null
  double *forms;         // [n][MEAS_FORMS + T], or null
  double *entropy;       // [n], or null
  const double *tab;     // [H * W + 2]; read only with entropy
  uint64_t *pack;        // [n][P][NW] the bit-plane image, or null
  unsigned long long *sum;       // with pack: [n / group], zeroed here for diversity_kernel's atomic adds
  unsigned long long *near_key;  // with pack: [n], set to all ones here for diversity_kernel's atomic mins
  int32_t group;
};

#ifdef __HIPCC__

__device__ __forceinline__ const uint8_t *meas_wave_stage(const MeasWaveArgs &a, const int e, uint8_t *cells) {
  const int lane = threadIdx.x;
  const uint8_t *src = a.grids + (size_t)e * a.stride;
  const int off = (int)((uintptr_t)src & 15u);
  const uint4 *s16 = (const uint4 *)(src - off);
  const int nv = (off + a.h * a.w + 15) >> 4;  // <= CAP / 16 + 1
  for (int i = lane; i < nv; i += 64) ((uint4 *)cells)[i] = s16[i];
  __syncthreads();
  return cells + off;
}

template <int T, int P>
__device__ __forceinline__ void meas_wave_body(const MeasWaveArgs &a, const int e, const uint8_t *m) {
  static_assert(T >= 1 && T <= (1 << P), "a counted id fits the planes");
  const int lane = threadIdx.x;
  const int H = a.h, W = a.w, n = H * W;
  constexpr int idmask = (1 << P) - 1;
  const bool want_counts = a.counts != nullptr || a.entropy != nullptr || a.forms != nullptr;
  const bool want_match = a.match != nullptr || a.forms != nullptr;
  const int dr = 64 / W, dc = 64 - dr * W;  // 64 cells further on: dr rows and dc columns (W > 64: 0 rows, 64 columns)
  uint32_t cnt[T] = {};
  uint32_t hor = 0, ver = 0, co = 0;
  uint64_t word[P] = {};  // lane w: word w of each plane
  int r = lane / W, c = lane - r * W;
  for (int ch = 0; ch < a.NW; ch++) {
    const int i = ch * 64 + lane;
    const bool ok = i < n;
    const int rr = ok ? r : 0, cc = ok ? c : 0;
    const int id = m[ok ? i : 0] & idmask;
    if (a.pack != nullptr) {
#pragma unroll
      for (int k = 0; k < P; k++) {
        const uint64_t w = __ballot(ok && ((id >> k) & 1));
        if (lane == ch) word[k] = w;
      }
    }
    if (want_counts) {
#pragma unroll
      for (int t = 0; t < T; t++) cnt[t] += (uint32_t)__popcll(__ballot(ok && id == t));
    }
    if (want_match) {
      const int up = rr == 0 ? H - 1 : rr - 1, down = rr == H - 1 ? 0 : rr + 1;
      const int left = cc == 0 ? W - 1 : cc - 1, right = cc == W - 1 ? 0 : cc + 1;
      hor += (uint32_t)__popcll(__ballot(ok && rr < H / 2 && (m[(H - 1 - rr) * W + cc] & idmask) == id));
      ver += (uint32_t)__popcll(__ballot(ok && cc < W / 2 && (m[rr * W + (W - 1 - cc)] & idmask) == id));
      co += (uint32_t)__popcll(__ballot(ok && (m[up * W + cc] & idmask) == id));
      co += (uint32_t)__popcll(__ballot(ok && (m[down * W + cc] & idmask) == id));
      co += (uint32_t)__popcll(__ballot(ok && (m[rr * W + left] & idmask) == id));
      co += (uint32_t)__popcll(__ballot(ok && (m[rr * W + right] & idmask) == id));
    }
    c += dc;  // dc < W for W <= 64 and dc = 64 < W above: one carry is enough
    r += dr;
    if (c >= W) {
      c -= W;
      r++;
    }
  }
  if (a.pack != nullptr && lane < a.NW) {
#pragma unroll
    for (int k = 0; k < P; k++) a.pack[((size_t)e * P + k) * a.NW + lane] = word[k];
  }
  if (lane != 0) return;
  if (a.counts != nullptr) {
#pragma unroll
    for (int t = 0; t < T; t++) a.counts[(size_t)e * T + t] = (int32_t)cnt[t];
  }
  if (a.match != nullptr) {
    a.match[(size_t)e * 3] = (int32_t)hor;
    a.match[(size_t)e * 3 + 1] = (int32_t)ver;
    a.match[(size_t)e * 3 + 2] = (int32_t)co;
  }
  if (a.forms != nullptr) {
    double *f = a.forms + (size_t)e * (MEAS_FORMS + T);
    const double ncells = (double)n, half = (double)(W * H) / 2.0;  // (17.5 for 5 x 7, 0.5 for 1 x 1: evolve.py:507, :540)
    const double hs = (double)hor / half, vs = (double)ver / half;
    f[0] = (double)cnt[0] / ncells;
    f[1] = hs;
    f[2] = vs;
    f[3] = (vs + hs) / 2.0;
    f[4] = (double)co / (double)(n * 4);
#pragma unroll
    for (int t = 0; t < T; t++) f[MEAS_FORMS + t] = (double)cnt[t] / ncells;
  }
  if (a.entropy != nullptr) {
    double ent = 0.0;
#pragma unroll
    for (int t = 0; t < T; t++)
      if (cnt[t] != 0) ent -= a.tab[cnt[t]];
    a.entropy[e] = ent / a.tab[n + 1];
  }
  if (a.pack != nullptr) {
    if (e % a.group == 0) a.sum[e / a.group] = 0ull;
    a.near_key[e] = ~0ull;
  }
}

template <int T, int P, int CAP>
__device__ __forceinline__ void meas_wave_map(const MeasWaveArgs &a, const int e, uint8_t *cells) {
  static_assert(CAP % 64 == 0 && CAP / 64 <= 64, "lane w keeps word w of each plane");
  meas_wave_body<T, P>(a, e, meas_wave_stage(a, e, cells));
}

#endif  // __HIPCC__

}  // namespace pcgrl
