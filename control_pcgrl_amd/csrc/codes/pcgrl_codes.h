// codes/pcgrl_codes.h -- the tile-code observation form (include/pcgrl_amd_codes.h): launchers of the kernels in
// codes/pcgrl_codes.hip, called by the host side (pcgrl_engine.hip).
//
// The form is the reference's Cropped integer map (wrappers.py:407-437: map + 1, zero padding, cropped to obs_window)
// stacked by ToImage (:140-150) with the static_builds plane where configured -- OneHotEncoding (:232-257) left out.
// Channel-last uint8, P planes per cell:
//   narrow / turtle  [N][OH][OW][P], P = 1 + static_tiles: 0 = outside the map, 1 + tile inside; the static mask (0 outside)
//   wide             [N][H][W][1]: the tile
//   3-D maze         [N][o0][o1][o2][1]: the index of the one-hot channel (0 out of bounds, 1 AIR, 2 DIRT, 3 path overlay)
#pragma once
#include <hip/hip_runtime.h>

#include "../pcgrl_common.h"

namespace pcgrl {

struct CodesArgs {
  uint8_t *out;  // [N][T] codes
  int32_t T;     // bytes per env
  int32_t P;     // planes per cell (1, or 2 with the static plane)
  int32_t wide;  // 1: the whole map, code = tile; 0: the cropped window, code = 1 + tile, 0 outside the map
  int32_t nt;    // non-temporal stores (the launch writes far more than the last-level cache holds)
  // filled in by launch_codes_observe
  int32_t pad_l;  // padded code rows (one plane): zero bytes in front of the W codes (a multiple of 4) ...
  int32_t rs;     // ... and the row stride (a multiple of 16); 0 = the generic kernel
  int32_t pre;    // binary 16 x 16, 32 x 32 window: also compute the pre-flooded component of the next edit cell
};

// from-state encoder of the 2-D problems (narrow, turtle, wide; static tiles; any act_window): what pcgrl_observe shows
hipError_t launch_codes_observe(const Params &p, int lpe, const CodesArgs &a, hipStream_t s);
// one-hot rows -> codes: n_rows rows of `cells` cells with C one-hot bytes each, of which the first CS are the one-hot code
// and the remaining C - CS are copied (P = 1 + C - CS planes out)
hipError_t launch_onehot_to_codes(const uint8_t *onehot, int64_t n_rows, int cells, int C, int CS, uint8_t *codes, hipStream_t s);

}  // namespace pcgrl
