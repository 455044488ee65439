// loderunner/pcgrl_k_loderunner.hip -- translation unit: the Lode Runner level kernel (see loderunner/pcgrl_loderunner.h).
#define PCGRL_KERNEL_TU
#include "pcgrl_loderunner.h"

namespace pcgrl {

hipError_t launch_loderunner(const LrArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(loderunner_kernel, dim3(lr_blocks(a.n, a.h, a.w)), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace pcgrl
