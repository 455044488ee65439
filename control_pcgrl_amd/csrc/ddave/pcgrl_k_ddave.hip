// ddave/pcgrl_k_ddave.hip -- translation unit: the Dangerous Dave level kernel and the measure / pack kernel of Dangerous Dave
// maps (see ddave/pcgrl_ddave.h).  The pairwise kernels are those of measures/pcgrl_k_measures.hip.
#define PCGRL_DD_KERNEL
#define PCGRL_PT_KERNEL  // the device half of playthrough/pcgrl_playthrough.h
#include "pcgrl_ddave.h"

namespace pcgrl {

hipError_t launch_ddave(const PtArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ddave_kernel, dim3(a.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_dd_measures(const MeasWaveArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(dd_measures_kernel, dim3(a.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace pcgrl
