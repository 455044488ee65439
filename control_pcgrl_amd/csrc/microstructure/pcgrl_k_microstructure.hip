// microstructure/pcgrl_k_microstructure.hip -- translation unit: the microstructure level kernel and the measure / pack kernel
// of microstructure maps (see microstructure/pcgrl_microstructure.h).  The pairwise kernels are those of
// measures/pcgrl_k_measures.hip.
#define PCGRL_MS_KERNEL
#include "pcgrl_microstructure.h"

namespace pcgrl {

hipError_t launch_microstructure(const MsArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(microstructure_kernel, dim3(a.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ms_measures(const MeasWaveArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ms_measures_kernel, dim3(a.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace pcgrl
