// loderunner/pcgrl_loderunner_measures.h -- level measures and the bit-plane image of Lode Runner maps on the device
// (include/pcgrl_amd_loderunner_measures.h): the quantities of measures/pcgrl_measures.h -- the integers behind the reference's
// behaviour characteristics (evo/evolve.py:423-592) and, through the image, behind div_calc (rl/evaluate_ctrl.py:42-48) and
// diversity_bonus (evo/evolve.py:1236-1244) -- for maps the 2-D engine does not hold: 1..16 rows x 1..32 columns of bytes, the
// shapes pcgrl_loderunner_evaluate takes.  T = 8 tile types, P = 3 planes, n = H * W <= 512 cells, NW = ceil(n / 64) <= 8 words
// per plane.  DESIGN.md section 27.
//
// lr_measures_kernel: one 64-lane wave per map; the per-map body is meas_wave_map<8, 3, 512> of
// measures/pcgrl_measures_wave.h (that header has the staging, the chunks and the outputs), 544 B of LDS.  The pairwise step is
// measures/pcgrl_measures.h's diversity_kernel / diversity_finish_kernel, launched as they are on the image written here: they
// are generic in P and NW and read only the image, the sums and the keys.
//
// Cases this shape range brings:
//   H == 1     under np.roll along axis 0 a cell is its own vertical neighbour, twice: both vertical comparisons match (2 per
//              cell); H / 2 == 0, so there are no horizontal-symmetry pairs and symmetry-horizontal is 0 / (W / 2).
//   W == 1     the same along axis 1: 2 horizontal matches per cell, no vertical-symmetry pairs.
//   W == 2     both horizontal rolls meet the same cell: a matching pair counts 2 from each of its cells (H == 2 likewise).
//   1 x 1      no symmetry pairs at all over the divisor W * H / 2 = 0.5: symmetry 0 / 0.5 = 0; all four co-occurance
//              comparisons are the cell against itself: 4 / 4 = 1.0.
//   odd H, W   the middle row / column is left out of the symmetry pairs, and the divisor W * H / 2 is a float division that
//              need not be an integer (5 x 7: 17.5): a perfectly symmetric map scores below 1.
//   H * W < 64   a single chunk whose lanes past the last cell contribute to no ballot; their partner reads go to cell 0.
//   H * W == 512 eight full chunks; lanes 0..7 each keep one word of every plane.
//   divisors   H * W, W * H / 2 and H * W * 4 are the map's own, not the 12 x 8 the problem's targets are frozen at: an env's
//              _prob._width / _height follow the map (adjust_param), and get_bc reads the map's shape.
// Tile ids are masked to 3 bits as every measures kernel here does.  With T = 8 every masked id is a counted tile, ids >= 8
// alias (9 counts as brick), and no error bit is set anywhere: the measures are functions of the bytes.  The evaluator's own
// convention -- an id above 7 reads as empty and sets bit 0 of its d_error -- is untouched and differs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../measures/pcgrl_measures.h"       // DivArgs, launch_diversity, launch_diversity_finish
#include "../measures/pcgrl_measures_wave.h"  // MeasWaveArgs, meas_wave_map
#include "pcgrl_loderunner.h"                 // LR_MAX_H, LR_MAX_W

namespace pcgrl {

constexpr int LR_MEAS_TILES = 8, LR_MEAS_PLANES = 3;
constexpr int LR_MEAS_MAX_CELLS = LR_MAX_H * LR_MAX_W;  // 512
constexpr int LR_MEAS_MAX_WORDS = LR_MEAS_MAX_CELLS / 64;  // 8

hipError_t launch_lr_measures(const MeasWaveArgs &a, hipStream_t s);

#ifdef PCGRL_LR_MEASURES_KERNEL  // (loderunner/pcgrl_k_loderunner_measures.hip has it)

__global__ __launch_bounds__(64) void lr_measures_kernel(const MeasWaveArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t cells[LR_MEAS_MAX_CELLS + 32];
  const int e = blockIdx.x;
  if (e >= a.n) return;
  meas_wave_map<LR_MEAS_TILES, LR_MEAS_PLANES, LR_MEAS_MAX_CELLS>(a, e, cells);
}

#endif  // PCGRL_LR_MEASURES_KERNEL

}  // namespace pcgrl
