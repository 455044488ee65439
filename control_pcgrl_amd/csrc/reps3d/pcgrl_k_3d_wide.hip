// reps3d/pcgrl_k_3d_wide.hip -- translation unit: the minecraft_3D_maze kernels of the wide representation (pcgrl_reps3d.h)
#define PCGRL_KERNEL_TU
#include "pcgrl_reps3d.h"

hipError_t pcgrl::launch_3d_wide(KernelId id, const Params &p, int cpl, hipStream_t s) {
  return launch_3d_rep<PCGRL_REP_WIDE>(id, p, cpl, s);
}
