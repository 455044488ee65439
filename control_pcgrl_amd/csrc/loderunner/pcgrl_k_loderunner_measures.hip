// loderunner/pcgrl_k_loderunner_measures.hip -- translation unit: the measure / pack kernel of Lode Runner maps (see
// loderunner/pcgrl_loderunner_measures.h).  The pairwise kernels are those of measures/pcgrl_k_measures.hip.
#define PCGRL_LR_MEASURES_KERNEL
#include "pcgrl_loderunner_measures.h"

namespace pcgrl {

hipError_t launch_lr_measures(const MeasWaveArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(lr_measures_kernel, dim3(a.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace pcgrl
