// smb/pcgrl_k_smb_env.hip -- translation unit: the Super Mario Bros environment kernels (see smb/pcgrl_smb_env.h).
#define PCGRL_KERNEL_TU
#define PCGRL_SMB_DEVICE_ONLY
#define PCGRL_SMB_CTRL_KERNELS
#include "pcgrl_smb_env.h"

namespace pcgrl {

hipError_t launch_smb_env(SmbEnvKernel k, const SmbEnvArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  switch (k) {
    case SMB_ENV_RESET:
      if (a.ctrl.rec) hipLaunchKernelGGL(smb_env_reset_kernel<true>, dim3(a.n), dim3(64), 0, s, a);
      else hipLaunchKernelGGL(smb_env_reset_kernel<false>, dim3(a.n), dim3(64), 0, s, a);
      break;
    case SMB_ENV_STEP:
      if (a.ctrl.rec) hipLaunchKernelGGL(smb_env_step_kernel<true>, dim3(a.n), dim3(64), 0, s, a);
      else hipLaunchKernelGGL(smb_env_step_kernel<false>, dim3(a.n), dim3(64), 0, s, a);
      break;
    case SMB_ENV_OBSERVE: hipLaunchKernelGGL(smb_env_observe_kernel, dim3(a.n), dim3(64), 0, s, a); break;
  }
  return hipGetLastError();
}

hipError_t launch_smb_env_gather(const SmbEnvGather &g, hipStream_t s) {
  if (g.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(smb_env_gather_kernel, dim3(g.n), dim3(64), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_smb_ctrl_queue(const SmbCtrlQueueArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(smb_ctrl_queue_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_smb_ctrl_get(const SmbCtrlGetArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(smb_ctrl_get_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_smb_ctrl_observe(const SmbCtrlObserveArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(smb_ctrl_observe_kernel, dim3((a.n * SMB_STATS + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_smb_ctrl_resample(const SmbCtrlResampleArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(smb_ctrl_resample_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace pcgrl
