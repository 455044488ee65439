// smb/pcgrl_k_smb_env.hip -- translation unit: the Super Mario Bros environment kernels (see smb/pcgrl_smb_env.h).
#define PCGRL_KERNEL_TU
#define PCGRL_SMB_DEVICE_ONLY
#include "pcgrl_smb_env.h"

namespace pcgrl {

hipError_t launch_smb_env(SmbEnvKernel k, const SmbEnvArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  switch (k) {
    case SMB_ENV_RESET: hipLaunchKernelGGL(smb_env_reset_kernel, dim3(a.n), dim3(64), 0, s, a); break;
    case SMB_ENV_STEP: hipLaunchKernelGGL(smb_env_step_kernel, dim3(a.n), dim3(64), 0, s, a); break;
    case SMB_ENV_OBSERVE: hipLaunchKernelGGL(smb_env_observe_kernel, dim3(a.n), dim3(64), 0, s, a); break;
  }
  return hipGetLastError();
}

hipError_t launch_smb_env_gather(const SmbEnvGather &g, hipStream_t s) {
  if (g.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(smb_env_gather_kernel, dim3(g.n), dim3(64), 0, s, g);
  return hipGetLastError();
}

}  // namespace pcgrl
