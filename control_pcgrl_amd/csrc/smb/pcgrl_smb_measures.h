// smb/pcgrl_smb_measures.h -- level measures and the bit-plane image of Super Mario Bros maps on the device
// (include/pcgrl_amd_smb_measures.h): the quantities of measures/pcgrl_measures.h -- the integers behind the reference's
// behaviour characteristics (evo/evolve.py:423-592) and, through the image, behind div_calc (rl/evaluate_ctrl.py:42-48) and
// diversity_bonus (evo/evolve.py:1236-1244) -- for maps the 2-D engine does not hold: 4..16 rows x 1..128 columns of bytes,
// T = 7 tile types, P = 3 planes, n = H * W <= 2 048 cells, NW = ceil(n / 64) <= 32 words per plane.  DESIGN.md section 24.
//
// The rules and the order of the double operations are those of measures/pcgrl_measures.h (its header comment states them;
// tests/measures_numpy.py is the same in numpy); the pairwise step is that file's diversity_kernel / diversity_finish_kernel,
// launched as they are on the image written here: they are generic in P and NW and read only the image, the sums and the keys.
// A 16-column tile of stock 16 x 116 maps is 16 x 3 x 29 x 8 = 11 136 bytes of their LDS.
//
// smb_measures_kernel: one 64-lane wave per map.  The map's bytes are staged in LDS with 16-byte loads from one of two sources:
//   caller maps   uint8 [n][H][W] at any alignment: the aligned 16-byte blocks that hold the map's first and last byte are read
//                 whole (as measures_kernel does), at most 129 loads;
//   env maps      the committed maps of an SMB env handle, rows of map_stride = H * W rounded up to 16 bytes, 16-byte aligned
//                 (smb_env_load_map of smb/pcgrl_smb_env.h).
// Per 64-cell chunk a lane holds one cell; __ballot((id >> p) & 1) IS word p of the chunk in the image ([map][P][NW] uint64, the
// tail lanes contribute 0), the counts and matches are popcounts of ballots and the partner cells come from LDS.  Lane w keeps
// word w of each plane, so the image leaves as three contiguous runs of NW words.  2 080 B of LDS.
//
// Cases the 2-D kernel (at most 64 x 64) never met:
//   W > 64     a 64-cell chunk is less than one row: a lane's cell moves on by 64 columns and at most one row (dr = 64 / W = 0,
//              dc = 64, one carry), and a row's mirror and neighbour cells lie in other chunks -- they come from LDS, which
//              holds the whole map, so nothing depends on the chunk.
//   W == 1     under np.roll a cell is its own horizontal neighbour, twice: both horizontal comparisons match (2 per cell);
//              W / 2 == 0, so there are no vertical-symmetry pairs and symmetry-vertical is 0 / (H / 2).
//   W == 2     both horizontal rolls meet the same cell: a matching pair counts 2 from each of its cells.
//   odd H, W   the middle row / column is left out of the symmetry pairs, and the divisor W * H / 2 is a float division that
//              need not be an integer (5 x 7: 17.5): a perfectly symmetric map scores below 1.
// Tile ids are masked to 3 bits as the existing measures do: id 7 matches no count but still compares, ids >= 8 alias, and no
// error bit is set (the measures are functions of the bytes; the evaluator's error bit is its own).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../measures/pcgrl_measures.h"  // MEAS_FORMS, DivArgs, launch_diversity, launch_diversity_finish
#include "pcgrl_smb.h"                   // SMB_MIN_H, SMB_MAX_H, SMB_MAX_W

namespace pcgrl {

constexpr int SMB_MEAS_TILES = 7, SMB_MEAS_PLANES = 3;
constexpr int SMB_MEAS_MAX_CELLS = SMB_MAX_H * SMB_MAX_W;  // 2 048
constexpr int SMB_MEAS_MAX_WORDS = SMB_MEAS_MAX_CELLS / 64;  // 32
static_assert(SMB_MEAS_MAX_WORDS <= 64, "smb_measures_kernel keeps word w of the image in lane w");

struct SmbMeasArgs {
  const uint8_t *grids;  // uint8 [n][H][W] caller maps at any alignment, or null: `maps`
  const uint8_t *maps;   // [n][map_stride], 16-byte aligned rows: an env handle's committed maps
  int32_t map_stride;
  int32_t h, w, n, NW;
  int32_t *counts;       // [n][7], or null
  int32_t *match;        // [n][3], or null
  double *forms;         // [n][MEAS_FORMS + 7], or null
  double *entropy;       // [n], or null
  const double *tab;     // [H * W + 2]; read only with entropy
  uint64_t *pack;        // [n][3][NW] the bit-plane image, or null
  unsigned long long *sum;       // with pack: [n / group], zeroed here for diversity_kernel's atomic adds
  unsigned long long *near_key;  // with pack: [n], set to all ones here for diversity_kernel's atomic mins
  int32_t group;
};

hipError_t launch_smb_measures(const SmbMeasArgs &a, hipStream_t s);

#ifdef PCGRL_SMB_MEASURES_KERNEL  // (smb/pcgrl_k_smb_measures.hip has it)

__global__ __launch_bounds__(64) void smb_measures_kernel(const SmbMeasArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t cells[SMB_MEAS_MAX_CELLS + 32];
  const int lane = threadIdx.x, e = blockIdx.x;
  if (e >= a.n) return;
  const int H = a.h, W = a.w, n = H * W;
  int off = 0;
  if (a.grids != nullptr) {
    const uint8_t *src = a.grids + (size_t)e * n;
    off = (int)((uintptr_t)src & 15u);
    const uint4 *s16 = (const uint4 *)(src - off);
    const int nv = (off + n + 15) >> 4;  // <= 129
    for (int i = lane; i < nv; i += 64) ((uint4 *)cells)[i] = s16[i];
  } else {
    const uint4 *s16 = (const uint4 *)(a.maps + (size_t)e * a.map_stride);
    for (int i = lane; i < a.map_stride / 16; i += 64) ((uint4 *)cells)[i] = s16[i];
  }
  __syncthreads();
  const uint8_t *m = cells + off;
  constexpr int T = SMB_MEAS_TILES, P = SMB_MEAS_PLANES, idmask = (1 << P) - 1;
  const bool want_counts = a.counts != nullptr || a.entropy != nullptr || a.forms != nullptr;
  const bool want_match = a.match != nullptr || a.forms != nullptr;
  const int dr = 64 / W, dc = 64 - dr * W;  // 64 cells further on: dr rows and dc columns (W > 64: 0 rows, 64 columns)
  uint32_t cnt[T] = {0, 0, 0, 0, 0, 0, 0};
  uint32_t hor = 0, ver = 0, co = 0;
  uint64_t word[P] = {0ull, 0ull, 0ull};  // lane w: word w of each plane
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
    const double ncells = (double)n, half = (double)(W * H) / 2.0;  // (17.5 for 5 x 7: evolve.py:507, :540)
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

#endif  // PCGRL_SMB_MEASURES_KERNEL

}  // namespace pcgrl
