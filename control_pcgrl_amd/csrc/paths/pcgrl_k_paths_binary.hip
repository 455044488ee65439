// paths/pcgrl_k_paths_binary.hip -- translation unit: the path kernels of the binary problem (see paths/pcgrl_paths.h).
#define PCGRL_KERNEL_TU
#include "pcgrl_paths.h"

namespace pcgrl {

hipError_t launch_paths_binary(const Params &p, int lpe, const PathArgs &a, hipStream_t s) {
  return launch_paths_prob<PCGRL_PROB_BINARY>(p, lpe, a, s);
}

}  // namespace pcgrl
