// mdungeon/pcgrl_k_mdungeon.hip -- translation unit: the MiniDungeon level kernel and the measure / pack kernel of MiniDungeon
// maps (see mdungeon/pcgrl_mdungeon.h).  The pairwise kernels are those of measures/pcgrl_k_measures.hip.
#define PCGRL_MD_KERNEL
#define PCGRL_PT_KERNEL  // the device half of playthrough/pcgrl_playthrough.h
#include "pcgrl_mdungeon.h"

namespace pcgrl {

hipError_t launch_mdungeon(const PtArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(mdungeon_kernel, dim3(a.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_md_measures(const MeasWaveArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(md_measures_kernel, dim3(a.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace pcgrl
