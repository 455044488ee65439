// smb/pcgrl_k_smb_state.hip -- translation unit: checkpoint and restore of Super Mario Bros environments (see
// smb/pcgrl_smb_state.h).
#define PCGRL_KERNEL_TU
#define PCGRL_SMB_DEVICE_ONLY
#define PCGRL_SMB_ENV_DEVICE_ONLY
#define PCGRL_SMB_READY_DEVICE_ONLY
#include "pcgrl_smb_state.h"

namespace pcgrl {

hipError_t launch_smb_state(SmbStateKernel k, const SmbStateArgs &a, hipStream_t s) {
  if (a.r.e.n <= 0) return hipSuccess;
  const dim3 grid(a.r.e.n), block(64);
  switch (k) {
    case SMB_STATE_EXPORT: hipLaunchKernelGGL(smb_state_export_kernel, grid, block, 0, s, a); break;
    case SMB_STATE_IMPORT: hipLaunchKernelGGL(smb_state_import_kernel, grid, block, 0, s, a); break;
    case SMB_STATE_SET:
      if (a.r.e.ctrl.rec) hipLaunchKernelGGL(smb_state_set_kernel<true>, grid, block, 0, s, a);
      else hipLaunchKernelGGL(smb_state_set_kernel<false>, grid, block, 0, s, a);
      break;
    case SMB_STATE_RNG: hipLaunchKernelGGL(smb_state_rng_kernel, grid, block, 0, s, a); break;
  }
  return hipGetLastError();
}

}  // namespace pcgrl
