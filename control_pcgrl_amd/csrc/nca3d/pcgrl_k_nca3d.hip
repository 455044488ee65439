// nca3d/pcgrl_k_nca3d.hip -- translation unit: the 3-D NCA level generator (see nca3d/pcgrl_nca3d.h) and the host side of
// include/pcgrl_amd_nca3d.h.  The unit stands alone: it has its own handle and its own last-error string.
#define PCGRL_NCA_KERNEL  // nca_layers23, nca_pick and nca_s32 of the 2-D generator
#define PCGRL_NCA3D_KERNEL
#include "pcgrl_nca3d.h"

#include <new>
#include <string>

#include "../../../include/pcgrl_amd_nca3d.h"

namespace pcgrl {

template <int T>
static hipError_t launch_nca3d_t(int64_t pairs, const Nca3dArgs &a, hipStream_t s) {
  const size_t lds = nca3d_lds_bytes(T, a.D0, a.D1, a.D2);
  hipLaunchKernelGGL((nca3d_kernel<T>), dim3((uint32_t)pairs), dim3(nca3d_threads(a.D0 * a.D1 * a.D2)), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_nca3d(int T, int64_t pairs, const Nca3dArgs &a, hipStream_t s) {
  switch (T) {
    case 2: return launch_nca3d_t<2>(pairs, a, s);
    case 3: return launch_nca3d_t<3>(pairs, a, s);
    case 4: return launch_nca3d_t<4>(pairs, a, s);
    case 5: return launch_nca3d_t<5>(pairs, a, s);
    case 6: return launch_nca3d_t<6>(pairs, a, s);
    case 7: return launch_nca3d_t<7>(pairs, a, s);
    case 8: return launch_nca3d_t<8>(pairs, a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace pcgrl

using namespace pcgrl;

namespace {

thread_local std::string g_nca3d_err;

int nca3d_fail(int code, const char *who, const std::string &msg) {
  g_nca3d_err = std::string(who) + ": " + msg;
  return code;
}

struct Nca3d {
  uint32_t tag;  // NCA3D_MAGIC while alive
  int32_t T, D0, D1, D2;
  int device;
  uint32_t *error;  // device, [1]
};

Nca3d *nca3d_of(void *p) {
  Nca3d *n = (Nca3d *)p;
  return n && n->tag == NCA3D_MAGIC ? n : nullptr;
}

bool axis_ok(int32_t d) { return d >= NCA3D_MIN_AXIS && d <= NCA3D_MAX_AXIS; }

}  // namespace

extern "C" {

const char *pcgrl_nca3d_last_error(void) { return g_nca3d_err.c_str(); }

int pcgrl_nca3d_create(int32_t n_tiles, int32_t d0, int32_t d1, int32_t d2, int32_t device, void **out) {
  const char *who = "pcgrl_nca3d_create";
  if (!out) return nca3d_fail(PCGRL_EINVAL, who, "out must not be null");
  *out = nullptr;
  if (n_tiles < NCA_MIN_T || n_tiles > NCA_MAX_T) return nca3d_fail(PCGRL_EINVAL, who, "the tile count must be in [2, 8]");
  if (!axis_ok(d0) || !axis_ok(d1) || !axis_ok(d2))
    return nca3d_fail(PCGRL_EINVAL, who, "every axis of the map must be in [3, 16]");
  if (device < 0) return nca3d_fail(PCGRL_EINVAL, who, "device must not be negative");
  Nca3d *n = new (std::nothrow) Nca3d();
  if (!n) return nca3d_fail(PCGRL_EHIP, who, "out of host memory");
  n->T = n_tiles, n->D0 = d0, n->D1 = d1, n->D2 = d2, n->device = device;
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
    return nca3d_fail(PCGRL_EHIP, who, std::string("allocating the error word: ") + hipGetErrorString(e));
  }
  n->tag = NCA3D_MAGIC;
  *out = n;
  return PCGRL_OK;
}

void pcgrl_nca3d_destroy(void *nca3d) {
  Nca3d *n = nca3d_of(nca3d);
  if (!n) return;
  n->tag = 0;
  (void)hipFree(n->error);
  delete n;
}

int pcgrl_nca3d_generate(void *nca3d, int32_t n_genomes, int32_t n_seeds, const float *d_weights, const uint8_t *d_init,
                         int32_t init_per_genome, const int32_t *d_holes, int32_t holes_per_seed, int32_t border_tile,
                         int32_t empty_tile, int32_t n_steps, uint8_t *d_levels, int32_t *d_n_step, uint8_t *d_frames,
                         void *stream) {
  const char *who = "pcgrl_nca3d_generate";
  Nca3d *n = nca3d_of(nca3d);
  if (!n) return nca3d_fail(PCGRL_EINVAL, who, "null or dead generator handle");
  if (n_genomes < 1 || n_seeds < 1) return nca3d_fail(PCGRL_EINVAL, who, "n_genomes and n_seeds must be at least 1");
  const int64_t pairs = (int64_t)n_genomes * n_seeds;
  if (pairs > 0x7FFFFFFF) return nca3d_fail(PCGRL_EINVAL, who, "n_genomes * n_seeds must be below 2^31");
  if (n_steps < 1 || n_steps > NCA_MAX_STEPS) return nca3d_fail(PCGRL_EINVAL, who, "n_steps must be in [1, 1024]");
  if (!d_weights || !d_init) return nca3d_fail(PCGRL_EINVAL, who, "d_weights and d_init must not be null");
  if (!d_levels || !d_n_step) return nca3d_fail(PCGRL_EINVAL, who, "d_levels and d_n_step must not be null");
  if (d_holes && (border_tile < 0 || border_tile >= n->T || empty_tile < 0 || empty_tile >= n->T))
    return nca3d_fail(PCGRL_EINVAL, who, "border_tile and empty_tile must be tiles below the tile count");
  Nca3dArgs k;
  k.D0 = n->D0, k.D1 = n->D1, k.D2 = n->D2, k.S = n_seeds, k.n_steps = n_steps, k.init_per_genome = init_per_genome != 0;
  k.holey = d_holes != nullptr, k.holes_per_seed = holes_per_seed != 0, k.border_tile = border_tile, k.empty_tile = empty_tile;
  k.weights = d_weights, k.init = d_init, k.holes = d_holes, k.levels = d_levels, k.n_step = d_n_step, k.frames = d_frames;
  k.error = n->error;
  hipError_t e = launch_nca3d(n->T, pairs, k, (hipStream_t)stream);
  if (e != hipSuccess) return nca3d_fail(PCGRL_EHIP, who, std::string("launching the kernel: ") + hipGetErrorString(e));
  return PCGRL_OK;
}

int pcgrl_nca3d_poll_error(void *nca3d, void *stream) {
  Nca3d *n = nca3d_of(nca3d);
  if (!n) {
    nca3d_fail(PCGRL_EINVAL, "pcgrl_nca3d_poll_error", "null or dead generator handle");
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  uint32_t bits = 0;
  hipError_t e = hipMemcpyAsync(&bits, n->error, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipMemsetAsync(n->error, 0, 4, s);
  if (e != hipSuccess) {
    nca3d_fail(PCGRL_EHIP, "pcgrl_nca3d_poll_error", hipGetErrorString(e));
    return -1;
  }
  return (int)bits;
}

}  // extern "C"
