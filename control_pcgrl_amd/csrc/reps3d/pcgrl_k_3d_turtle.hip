// reps3d/pcgrl_k_3d_turtle.hip -- translation unit: the minecraft_3D_maze kernels of the turtle representation (pcgrl_reps3d.h)
#define PCGRL_KERNEL_TU
#include "pcgrl_reps3d.h"

hipError_t pcgrl::launch_3d_turtle(KernelId id, const Params &p, int cpl, hipStream_t s) {
  return launch_3d_rep<PCGRL_REP_TURTLE>(id, p, cpl, s);
}
