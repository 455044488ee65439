// smb/pcgrl_k_smb_vector.hip -- translation unit: the float32 hand-out of Super Mario Bros environments (see
// smb/pcgrl_smb_vector.h).
#define PCGRL_SMB_VECTOR_KERNEL
#include "pcgrl_smb_vector.h"

#include <algorithm>

namespace pcgrl {

hipError_t launch_smb_vector_obs(const SmbVectorArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  // slices of an env's run: about 2 048 waves in flight, never more slices than the run has passes of 256 floats
  const int passes = (a.oh * a.ow * (2 * a.n_ctrl + 8) + 255) / 256;
  const int slices = std::max(1, std::min(std::min(passes, 256), 2048 / a.n));
  hipLaunchKernelGGL(smb_vector_obs_kernel, dim3(a.n, slices), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace pcgrl
