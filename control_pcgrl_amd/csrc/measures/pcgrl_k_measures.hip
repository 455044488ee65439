// measures/pcgrl_k_measures.hip -- translation unit: the measure / pack kernel and the pairwise Hamming kernel
// (see measures/pcgrl_measures.h).
#define PCGRL_KERNEL_TU
#include "pcgrl_measures.h"

namespace pcgrl {

hipError_t launch_measures(const Params &p, const MeasWaveArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const dim3 grid(a.n), block(64);
  switch (p.n_tiles) {  // binary; sokoban; zelda
    case 2: hipLaunchKernelGGL((measures_kernel<2, 1>), grid, block, 0, s, p, a); break;
    case 5: hipLaunchKernelGGL((measures_kernel<5, 3>), grid, block, 0, s, p, a); break;
    case 8: hipLaunchKernelGGL((measures_kernel<8, 3>), grid, block, 0, s, p, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_diversity(const DivArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const dim3 grid((a.n / a.K) * ((a.K + 63) / 64) * a.splits), block(64);
  const size_t lds = (size_t)DIV_TC * a.P * a.NW * sizeof(uint64_t);  // <= 24 KB
  switch (a.P) {  // binary: 1 plane; zelda, sokoban: 3
    case 1: hipLaunchKernelGGL(diversity_kernel<1>, grid, block, lds, s, a); break;
    case 3: hipLaunchKernelGGL(diversity_kernel<3>, grid, block, lds, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_diversity_finish(const DivArgs &a, int32_t n_cells, int32_t *nearest, int32_t *nearest_idx, double *scores,
                                   hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(diversity_finish_kernel, dim3((a.n + 63) / 64), dim3(64), 0, s, a, n_cells, nearest, nearest_idx, scores);
  return hipGetLastError();
}

}  // namespace pcgrl
