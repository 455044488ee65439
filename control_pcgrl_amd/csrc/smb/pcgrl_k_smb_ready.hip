// smb/pcgrl_k_smb_ready.hip -- translation unit: asynchronous stepping of Super Mario Bros environments (see
// smb/pcgrl_smb_ready.h).
#define PCGRL_KERNEL_TU
#define PCGRL_SMB_DEVICE_ONLY
#define PCGRL_SMB_ENV_DEVICE_ONLY
#include "pcgrl_smb_ready.h"

namespace pcgrl {

hipError_t launch_smb_ready_step(const SmbReadyArgs &a, hipStream_t s) {
  if (a.e.n <= 0) return hipSuccess;
  if (a.e.ctrl.rec) hipLaunchKernelGGL(smb_ready_step_kernel<true>, dim3(a.e.n), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(smb_ready_step_kernel<false>, dim3(a.e.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_smb_ready_reset(const SmbReadyArgs &a, hipStream_t s) {
  if (a.e.n <= 0) return hipSuccess;
  if (a.e.ctrl.rec) hipLaunchKernelGGL(smb_ready_reset_kernel<true>, dim3(a.e.n), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(smb_ready_reset_kernel<false>, dim3(a.e.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_smb_ready_busy(const SmbPark *park, int n, uint8_t *busy, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(smb_ready_busy_kernel, dim3((n + 255) / 256), dim3(256), 0, s, park, n, busy);
  return hipGetLastError();
}

}  // namespace pcgrl
