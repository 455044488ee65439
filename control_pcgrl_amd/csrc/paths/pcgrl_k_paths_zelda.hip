// paths/pcgrl_k_paths_zelda.hip -- translation unit: the path kernels of the zelda problem (see paths/pcgrl_paths.h).
#define PCGRL_KERNEL_TU
#include "pcgrl_paths.h"

namespace pcgrl {

hipError_t launch_paths_zelda(const Params &p, int lpe, const PathArgs &a, hipStream_t s) {
  return launch_paths_prob<PCGRL_PROB_ZELDA>(p, lpe, a, s);
}

}  // namespace pcgrl
