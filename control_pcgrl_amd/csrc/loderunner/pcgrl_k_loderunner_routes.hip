// loderunner/pcgrl_k_loderunner_routes.hip -- translation unit: the Lode Runner routes kernel (see
// loderunner/pcgrl_loderunner_routes.h).  loderunner_kernel itself lives in pcgrl_k_loderunner.hip.
#define PCGRL_KERNEL_TU
#define PCGRL_LR_DEVICE_ONLY
#include "pcgrl_loderunner_routes.h"

namespace pcgrl {

hipError_t launch_loderunner_routes(const LrRouteArgs &a, hipStream_t s) {
  if (a.lr.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(loderunner_routes_kernel, dim3(lr_blocks(a.lr.n, a.lr.h, a.lr.w)), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace pcgrl
