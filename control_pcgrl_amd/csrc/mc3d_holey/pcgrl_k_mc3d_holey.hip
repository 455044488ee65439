// mc3d_holey/pcgrl_k_mc3d_holey.hip -- translation unit: the kernel of the 3-D holey dungeon and maze levels (see
// mc3d_holey/pcgrl_mc3d_holey.h).
#define PCGRL_H3_KERNEL
#include "pcgrl_mc3d_holey.h"

namespace pcgrl {

hipError_t launch_mc3d_holey(const H3Args &a, int blocks, hipStream_t s) {
  if (a.n <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(mc3d_holey_kernel, dim3(blocks), dim3(H3_THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace pcgrl
