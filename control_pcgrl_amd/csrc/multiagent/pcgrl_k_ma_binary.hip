// multiagent/pcgrl_k_ma_binary.hip -- translation unit: the multi-agent kernels of the binary problem (see
// multiagent/pcgrl_multiagent.h).
#define PCGRL_KERNEL_TU
#include "pcgrl_multiagent.h"

namespace pcgrl {

hipError_t launch_ma_binary(MaKernel k, const Params &p, int lpe, const MaArgs &a, size_t lds, hipStream_t s) {
  return launch_ma_prob<PCGRL_PROB_BINARY>(k, p, lpe, a, lds, s);
}

}  // namespace pcgrl
