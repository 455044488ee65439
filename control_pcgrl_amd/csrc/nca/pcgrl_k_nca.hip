// nca/pcgrl_k_nca.hip -- translation unit: the NCA level generator (see nca/pcgrl_nca.h) and the host side of
// include/pcgrl_amd_nca.h.  The unit stands alone: it has its own handle and its own last-error string.
#define PCGRL_NCA_KERNEL
#include "pcgrl_nca.h"

#include <new>
#include <string>

#include "../../../include/pcgrl_amd_nca.h"

namespace pcgrl {

template <int T>
static hipError_t launch_nca_t(int64_t pairs, const NcaArgs &a, hipStream_t s) {
  const int cells = a.H * a.W;
  const size_t lds = nca_lds_bytes(T, cells);
  // one cell per lane: two halve the broadcast reads of layer 2 but cost three of seven waves per SIMD, and measured slower
  // (-DPCGRL_NCA_TWO_CELLS is the development build of that A/B, loaded through PCGRL_LIB)
#ifdef PCGRL_NCA_TWO_CELLS
  const int cpl = cells > 64 ? 2 : 1;
#else
  const int cpl = 1;
#endif
  int threads = ((cells + cpl - 1) / cpl + 63) / 64 * 64;
  if (threads > NCA_MAX_THREADS) threads = NCA_MAX_THREADS;
  if (cpl == 2)
    hipLaunchKernelGGL((nca_kernel<T, 2>), dim3((uint32_t)pairs), dim3(threads), lds, s, a);
  else
    hipLaunchKernelGGL((nca_kernel<T, 1>), dim3((uint32_t)pairs), dim3(threads), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_nca(int T, int64_t pairs, const NcaArgs &a, hipStream_t s) {
  switch (T) {
    case 2: return launch_nca_t<2>(pairs, a, s);
    case 3: return launch_nca_t<3>(pairs, a, s);
    case 4: return launch_nca_t<4>(pairs, a, s);
    case 5: return launch_nca_t<5>(pairs, a, s);
    case 6: return launch_nca_t<6>(pairs, a, s);
    case 7: return launch_nca_t<7>(pairs, a, s);
    case 8: return launch_nca_t<8>(pairs, a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace pcgrl

using namespace pcgrl;

namespace {

thread_local std::string g_nca_err;

int nca_fail(int code, const char *who, const std::string &msg) {
  g_nca_err = std::string(who) + ": " + msg;
  return code;
}

struct Nca {
  uint32_t tag;  // NCA_MAGIC while alive
  int32_t T, H, W;
  int device;
  uint32_t *error;  // device, [1]
};

Nca *nca_of(void *p) {
  Nca *n = (Nca *)p;
  return n && n->tag == NCA_MAGIC ? n : nullptr;
}

}  // namespace

extern "C" {

const char *pcgrl_nca_last_error(void) { return g_nca_err.c_str(); }

int pcgrl_nca_create(int32_t n_tiles, int32_t height, int32_t width, int32_t device, void **out) {
  const char *who = "pcgrl_nca_create";
  if (!out) return nca_fail(PCGRL_EINVAL, who, "out must not be null");
  *out = nullptr;
  if (n_tiles < NCA_MIN_T || n_tiles > NCA_MAX_T) return nca_fail(PCGRL_EINVAL, who, "the tile count must be in [2, 8]");
  if (height < 1 || height > NCA_MAX_SIDE || width < 1 || width > NCA_MAX_SIDE)
    return nca_fail(PCGRL_EINVAL, who, "the map's height and width must be in [1, 64]");
  if (device < 0) return nca_fail(PCGRL_EINVAL, who, "device must not be negative");
  Nca *n = new (std::nothrow) Nca();
  if (!n) return nca_fail(PCGRL_EHIP, who, "out of host memory");
  n->T = n_tiles, n->H = height, n->W = width, n->device = device;
  int prev = 0;
  hipError_t e = hipGetDevice(&prev);
  if (e == hipSuccess) e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc((void **)&n->error, 256);
  if (e == hipSuccess) {
    e = hipMemset(n->error, 0, 256);
    if (e != hipSuccess) (void)hipFree(n->error);
  }
  (void)hipSetDevice(prev);
  if (e != hipSuccess) {
    delete n;
    return nca_fail(PCGRL_EHIP, who, std::string("allocating the error word: ") + hipGetErrorString(e));
  }
  n->tag = NCA_MAGIC;
  *out = n;
  return PCGRL_OK;
}

void pcgrl_nca_destroy(void *nca) {
  Nca *n = nca_of(nca);
  if (!n) return;
  n->tag = 0;
  (void)hipFree(n->error);
  delete n;
}

int pcgrl_nca_generate(void *nca, int32_t n_genomes, int32_t n_seeds, const float *d_weights, const uint8_t *d_init,
                       int32_t init_per_genome, int32_t n_steps, uint8_t *d_levels, int32_t *d_n_step, uint8_t *d_frames,
                       void *stream) {
  const char *who = "pcgrl_nca_generate";
  Nca *n = nca_of(nca);
  if (!n) return nca_fail(PCGRL_EINVAL, who, "null or dead generator handle");
  if (n_genomes < 1 || n_seeds < 1) return nca_fail(PCGRL_EINVAL, who, "n_genomes and n_seeds must be at least 1");
  const int64_t pairs = (int64_t)n_genomes * n_seeds;
  if (pairs > 0x7FFFFFFF) return nca_fail(PCGRL_EINVAL, who, "n_genomes * n_seeds must be below 2^31");
  if (n_steps < 1 || n_steps > NCA_MAX_STEPS) return nca_fail(PCGRL_EINVAL, who, "n_steps must be in [1, 1024]");
  if (!d_weights || !d_init) return nca_fail(PCGRL_EINVAL, who, "d_weights and d_init must not be null");
  if (!d_levels || !d_n_step) return nca_fail(PCGRL_EINVAL, who, "d_levels and d_n_step must not be null");
  NcaArgs k;
  k.H = n->H, k.W = n->W, k.S = n_seeds, k.n_steps = n_steps, k.init_per_genome = init_per_genome != 0;
  k.weights = d_weights, k.init = d_init, k.levels = d_levels, k.n_step = d_n_step, k.frames = d_frames, k.error = n->error;
  hipError_t e = launch_nca(n->T, pairs, k, (hipStream_t)stream);
  if (e != hipSuccess) return nca_fail(PCGRL_EHIP, who, std::string("launching the kernel: ") + hipGetErrorString(e));
  return PCGRL_OK;
}

int pcgrl_nca_poll_error(void *nca, void *stream) {
  Nca *n = nca_of(nca);
  if (!n) {
    nca_fail(PCGRL_EINVAL, "pcgrl_nca_poll_error", "null or dead generator handle");
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  uint32_t bits = 0;
  hipError_t e = hipMemcpyAsync(&bits, n->error, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipMemsetAsync(n->error, 0, 4, s);
  if (e != hipSuccess) {
    nca_fail(PCGRL_EHIP, "pcgrl_nca_poll_error", hipGetErrorString(e));
    return -1;
  }
  return (int)bits;
}

}  // extern "C"
