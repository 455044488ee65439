// smb/pcgrl_k_smb_rollout.hip -- translation unit: open-loop rollouts of Super Mario Bros environments and the device-drawn
// actions (see smb/pcgrl_smb_rollout.h).
#define PCGRL_KERNEL_TU
#define PCGRL_SMB_DEVICE_ONLY
#define PCGRL_SMB_ENV_DEVICE_ONLY
#include "pcgrl_smb_rollout.h"

namespace pcgrl {

hipError_t launch_smb_env_rollout(const SmbRolloutArgs &a, hipStream_t s) {
  if (a.e.n <= 0 || a.n_steps <= 0) return hipSuccess;
  if (a.e.ctrl.rec) hipLaunchKernelGGL(smb_env_rollout_kernel<true>, dim3(a.e.n), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(smb_env_rollout_kernel<false>, dim3(a.e.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_smb_env_sample(int32_t *out, int n, int n_actions, uint64_t seed, SmbDrawState *draw, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(smb_env_sample_kernel, dim3((n + 255) / 256), dim3(256), 0, s, out, n, (uint32_t)n_actions, seed, draw);
  return hipGetLastError();
}

}  // namespace pcgrl
