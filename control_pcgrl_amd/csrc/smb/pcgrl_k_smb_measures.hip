// smb/pcgrl_k_smb_measures.hip -- translation unit: the measure / pack kernel of Super Mario Bros maps (see
// smb/pcgrl_smb_measures.h).  The pairwise kernels are those of measures/pcgrl_k_measures.hip.
#define PCGRL_SMB_MEASURES_KERNEL
#include "pcgrl_smb_measures.h"

namespace pcgrl {

hipError_t launch_smb_measures(const MeasWaveArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(smb_measures_kernel, dim3(a.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace pcgrl
