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
// smb_measures_kernel: one 64-lane wave per map; the per-map body is meas_wave_map<7, 3, 2048> of
// measures/pcgrl_measures_wave.h (that header has the staging, the chunks and the outputs), 2 080 B of LDS.  The map's bytes
// come from one of the two sources that header takes:
//   caller maps   uint8 [n][H][W] at any alignment, stride = H * W: at most 129 loads;
//   env maps      the committed maps of an SMB env handle, stride = map_stride = H * W rounded up to 16 bytes, 16-byte aligned
//                 (smb_env_load_map of smb/pcgrl_smb_env.h): map_stride / 16 loads, none outside the handle's rows.
// Lane w keeps word w of each plane, so the image leaves as three contiguous runs of NW words.
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

#include "../measures/pcgrl_measures.h"       // DivArgs, launch_diversity, launch_diversity_finish
#include "../measures/pcgrl_measures_wave.h"  // MeasWaveArgs, meas_wave_map
#include "pcgrl_smb.h"                        // SMB_MIN_H, SMB_MAX_H, SMB_MAX_W

namespace pcgrl {

constexpr int SMB_MEAS_TILES = 7, SMB_MEAS_PLANES = 3;
constexpr int SMB_MEAS_MAX_CELLS = SMB_MAX_H * SMB_MAX_W;  // 2 048
constexpr int SMB_MEAS_MAX_WORDS = SMB_MEAS_MAX_CELLS / 64;  // 32
static_assert(SMB_MEAS_MAX_WORDS <= 64, "smb_measures_kernel keeps word w of the image in lane w");

hipError_t launch_smb_measures(const MeasWaveArgs &a, hipStream_t s);

#ifdef PCGRL_SMB_MEASURES_KERNEL  // (smb/pcgrl_k_smb_measures.hip has it)

__global__ __launch_bounds__(64) void smb_measures_kernel(const MeasWaveArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t cells[SMB_MEAS_MAX_CELLS + 32];
  const int e = blockIdx.x;
  if (e >= a.n) return;
  meas_wave_map<SMB_MEAS_TILES, SMB_MEAS_PLANES, SMB_MEAS_MAX_CELLS>(a, e, cells);
}

#endif  // PCGRL_SMB_MEASURES_KERNEL

}  // namespace pcgrl
