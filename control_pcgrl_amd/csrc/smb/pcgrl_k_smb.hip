// smb/pcgrl_k_smb.hip -- translation unit: the Super Mario Bros level kernel (see smb/pcgrl_smb.h).
#define PCGRL_KERNEL_TU
#include "pcgrl_smb.h"

namespace pcgrl {

hipError_t launch_smb(const SmbArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(smb_kernel, dim3(a.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace pcgrl
