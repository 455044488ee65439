// solutions/pcgrl_k_solutions.hip -- translation unit: the Sokoban solution kernels (see solutions/pcgrl_solutions.h), one
// per (lanes per map, row-mask width) form validate() can choose, each from the engine's planes and from caller bytes.
#define PCGRL_KERNEL_TU
#include "pcgrl_solutions.h"

namespace pcgrl {

hipError_t launch_solutions(const Params &p, int lpe, const SolArgs &a, hipStream_t s) {
  if (p.n_envs <= 0) return hipSuccess;
  if (p.cfg.problem != PCGRL_PROB_SOKOBAN || p.soko == nullptr) return hipErrorInvalidValue;
  if (p.cfg.dims[1] > 32) {  // 64-bit row masks: 32 or 64 lanes per map (validate())
    if (lpe == 32) return launch_solutions_pl<32, uint64_t>(p, a, s);
    return launch_solutions_pl<64, uint64_t>(p, a, s);
  }
  switch (lpe) {
    case 8: return launch_solutions_pl<8, uint32_t>(p, a, s);
    case 16: return launch_solutions_pl<16, uint32_t>(p, a, s);
    case 32: return launch_solutions_pl<32, uint32_t>(p, a, s);
    default: return launch_solutions_pl<64, uint32_t>(p, a, s);
  }
}

}  // namespace pcgrl
