// async3d/pcgrl_k_3d_async.hip -- translation unit: the asynchronous-stepping kernels of minecraft_3D_maze (pcgrl_async3d.h)
#define PCGRL_KERNEL_TU
#include "pcgrl_async3d.h"

hipError_t pcgrl::launch_3d_async(KernelId id, const Params &p, int cpl, hipStream_t s) { return launch_3d_async_impl(id, p, cpl, s); }

hipError_t pcgrl::launch_3d_async_unpark(void *pool, int Z, int Y, int X, int n_envs, const uint8_t *mask, hipStream_t s) {
  const int words = m3_size_class(Z, Y, X) == 0 ? A3P<0>::WORDS : A3P<1>::WORDS;
  hipLaunchKernelGGL(a3_unpark_kernel, dim3((n_envs + 255) / 256), dim3(256), 0, s, (uint32_t *)pool, words, n_envs, mask);
  return hipGetLastError();
}
