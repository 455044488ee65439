// archive/pcgrl_k_archive.hip -- translation unit: the quality-diversity grid archive (see archive/pcgrl_archive.h) and the
// host side of include/pcgrl_amd_archive.h.  The unit stands alone: it has its own handle and its own last-error string.
#define PCGRL_ARCHIVE_KERNEL
#include "pcgrl_archive.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "../../../include/pcgrl_amd_archive.h"
#include "../../../include/pcgrl_amd_evo.h"
#include "../evo/pcgrl_evo.h"

namespace pcgrl {

static inline int arch_blocks(int64_t threads) { return (int)((threads + 255) / 256); }

hipError_t launch_arch_add(const ArchAddArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(arch_key_kernel, dim3(arch_blocks(a.n)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(arch_winner_kernel, dim3(arch_blocks(a.n)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(arch_status_kernel, dim3(arch_blocks(a.n)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(arch_commit_kernel, dim3((a.n + 3) / 4), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_arch_cells(const ArchGrid &g, int32_t n, const double *beh, int32_t *cell, hipStream_t s) {
  hipLaunchKernelGGL(arch_cells_kernel, dim3(arch_blocks(n)), dim3(256), 0, s, g, n, beh, cell);
  return hipGetLastError();
}

hipError_t launch_arch_scan(const ArchGrid &g, const ArchMem &m, int32_t *counts, hipStream_t s) {
  hipLaunchKernelGGL(arch_scan_kernel, dim3(1), dim3(ARCH_SCAN_THREADS), 0, s, g, m, counts);
  return hipGetLastError();
}

hipError_t launch_arch_stats(const ArchMem &m, double *out, hipStream_t s) {
  hipLaunchKernelGGL(arch_stats_kernel, dim3(1), dim3(64), 0, s, m, out);
  return hipGetLastError();
}

hipError_t launch_arch_elites(const ArchElitesArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(arch_elites_kernel, dim3(arch_blocks((int64_t)a.cap * a.g.L)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_arch_ask(const ArchAskArgs &a, hipStream_t s) {
  const int block = a.g.L >= 256 ? 256 : (a.g.L + 63) / 64 * 64;
  hipLaunchKernelGGL(arch_ask_kernel, dim3(a.n, (a.g.L + block - 1) / block), dim3(block), 0, s, a);
  hipLaunchKernelGGL(arch_bump_kernel, dim3(1), dim3(64), 0, s, a.m);
  return hipGetLastError();
}

hipError_t launch_arch_clear(const ArchGrid &g, const ArchMem &m, hipStream_t s) {
  hipLaunchKernelGGL(arch_clear_kernel, dim3(arch_blocks(g.cells)), dim3(256), 0, s, g, m);
  return hipGetLastError();
}

hipError_t launch_arch_export_header(const ArchGrid &g, const ArchMem &m, void *image, hipStream_t s) {
  hipLaunchKernelGGL(arch_export_header_kernel, dim3(1), dim3(64), 0, s, g, m, (ArchHeader *)image);
  return hipGetLastError();
}

hipError_t launch_arch_import_finish(const ArchGrid &g, const ArchMem &m, const void *image, hipStream_t s) {
  hipLaunchKernelGGL(arch_import_finish_kernel, dim3(arch_blocks(g.cells)), dim3(256), 0, s, g, m, (const ArchHeader *)image);
  return hipGetLastError();
}

hipError_t launch_evo_children(const EvoChildrenArgs &a, hipStream_t s) {
  const int per = (a.P + EVO_EPT - 1) / EVO_EPT;  // threads that have an element
  const int block = per >= EVO_BLOCK ? EVO_BLOCK : (per + 63) / 64 * 64;
  hipLaunchKernelGGL(evo_children_kernel, dim3(a.n, (a.P + block * EVO_EPT - 1) / (block * EVO_EPT)), dim3(block), 0, s, a);
  hipLaunchKernelGGL(evo_bump_kernel, dim3(1), dim3(64), 0, s, a.m, a.with_parent);
  return hipGetLastError();
}

hipError_t launch_evo_aggregate(const EvoAggregateArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(evo_aggregate_kernel, dim3((a.G + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace pcgrl

using namespace pcgrl;

namespace {

thread_local std::string g_arch_err;

int arch_fail(int code, const char *who, const std::string &msg) {
  g_arch_err = std::string(who) + ": " + msg;
  return code;
}

#define ARCH_HIPCHK(expr)                                                                     \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return arch_fail(PCGRL_EHIP, who, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct Archive {
  uint32_t tag;  // ARCH_MAGIC while alive
  ArchGrid g;
  ArchMem m;
  int device;
  void *block;
};

inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }
inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// the sections of an image after the header: objectives, behaviours, map rows, flags
struct ImageLayout {
  size_t obj, beh, maps, flag, total;
};
ImageLayout image_layout(const ArchGrid &g) {
  ImageLayout l;
  l.obj = ARCH_HEADER_BYTES;
  l.beh = l.obj + up16((size_t)g.cells * 8);
  l.maps = l.beh + up16((size_t)g.cells * g.D * 8);
  l.flag = l.maps + (size_t)g.cells * g.LP;
  l.total = l.flag + up16((size_t)g.cells);
  return l;
}

Archive *arch_of(void *p) {
  Archive *a = (Archive *)p;
  return a && a->tag == ARCH_MAGIC ? a : nullptr;
}

}  // namespace

extern "C" {

const char *pcgrl_archive_last_error(void) { return g_arch_err.c_str(); }

// map_bytes and n_tiles of a map archive, or 4 * n_params and 0 of a genome archive (already checked by the caller)
static int arch_create(const char *who, int32_t n_axes, const int32_t *dims, const double *lo, const double *hi, int32_t map_bytes,
                       int32_t n_tiles, int32_t device, void **out) {
  if (!dims || !lo || !hi || !out) return arch_fail(PCGRL_EINVAL, who, "dims, lo, hi and out must not be null");
  *out = nullptr;
  if (n_axes < 1 || n_axes > ARCH_MAX_AXES) return arch_fail(PCGRL_EINVAL, who, "the number of behaviour axes must be in [1, 4]");
  int64_t cells = 1;
  for (int j = 0; j < n_axes; j++) {
    if (dims[j] < 1) return arch_fail(PCGRL_EINVAL, who, "every dim must be at least 1");
    cells *= dims[j];
    if (cells > ARCH_MAX_CELLS) return arch_fail(PCGRL_EINVAL, who, "more than 2^20 cells");
    if (!std::isfinite(lo[j]) || !std::isfinite(hi[j])) return arch_fail(PCGRL_EINVAL, who, "the bounds must be finite");
    if (!(lo[j] < hi[j])) return arch_fail(PCGRL_EINVAL, who, "every axis needs lo < hi");
  }
  if (n_tiles > 0 && (map_bytes < 1 || map_bytes > ARCH_MAX_L))
    return arch_fail(PCGRL_EINVAL, who, "the map length must be in [1, 4096] bytes");
  if (n_tiles > ARCH_MAX_T) return arch_fail(PCGRL_EINVAL, who, "the tile count must be in [1, 256]");
  if (n_tiles == 0 && (uint64_t)cells * (uint64_t)((map_bytes + 15) / 16 * 16) > (1ull << 32))
    return arch_fail(PCGRL_EINVAL, who, "cells x row bytes is above 2^32");
  if (device < 0) return arch_fail(PCGRL_EINVAL, who, "device must not be negative");

  Archive *a = new (std::nothrow) Archive();
  if (!a) return arch_fail(PCGRL_EHIP, who, "out of host memory");
  ArchGrid &g = a->g;
  g.D = n_axes, g.cells = (int32_t)cells, g.L = map_bytes, g.LP = (map_bytes + 15) / 16 * 16, g.T = n_tiles;
  for (int j = 0; j < ARCH_MAX_AXES; j++) {
    g.dims[j] = j < n_axes ? dims[j] : 1;
    g.lo[j] = j < n_axes ? lo[j] : 0.0;
    g.hi[j] = j < n_axes ? hi[j] : 1.0;
  }
  a->device = device;
  const size_t n = (size_t)cells;
  const size_t o_obj = 0, o_beh = o_obj + up256(n * 8), o_word = o_beh + up256(n * g.D * 8), o_maps = o_word + up256(n * 8),
               o_win = o_maps + up256(n * g.LP), o_occ = o_win + up256(n * 4), o_flag = o_occ + up256(n * 4),
               o_misc = o_flag + up256(n), total = o_misc + 256;
  int prev = 0;
  hipError_t e = hipGetDevice(&prev);
  if (e == hipSuccess) e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc(&a->block, total);
  if (e != hipSuccess) {
    delete a;
    (void)hipSetDevice(prev);
    return arch_fail(PCGRL_EHIP, who, std::string("allocating the archive: ") + hipGetErrorString(e));
  }
  uint8_t *b = (uint8_t *)a->block;
  ArchMem &m = a->m;
  m.obj = (double *)(b + o_obj), m.beh = (double *)(b + o_beh), m.word = (uint64_t *)(b + o_word), m.maps = b + o_maps;
  m.win = (int32_t *)(b + o_win), m.occ = (int32_t *)(b + o_occ), m.flag = b + o_flag;
  m.stats_d = (double *)(b + o_misc), m.draw = (uint64_t *)(b + o_misc + 32), m.stats_i = (int32_t *)(b + o_misc + 48);
  m.error = (uint32_t *)(b + o_misc + 64);
  e = launch_arch_clear(g, m, nullptr);
  if (e == hipSuccess) e = launch_arch_scan(g, m, nullptr, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    (void)hipFree(a->block);
    delete a;
    (void)hipSetDevice(prev);
    return arch_fail(PCGRL_EHIP, who, std::string("clearing the archive: ") + hipGetErrorString(e));
  }
  (void)hipSetDevice(prev);
  a->tag = ARCH_MAGIC;
  *out = a;
  return PCGRL_OK;
}

int pcgrl_archive_create(int32_t n_axes, const int32_t *dims, const double *lo, const double *hi, int32_t map_bytes,
                         int32_t n_tiles, int32_t device, void **out) {
  const char *who = "pcgrl_archive_create";
  if (out) *out = nullptr;
  if (n_tiles < 1) return arch_fail(PCGRL_EINVAL, who, "the tile count must be in [1, 256]");
  return arch_create(who, n_axes, dims, lo, hi, map_bytes, n_tiles, device, out);
}

int pcgrl_archive_create_genomes(int32_t n_axes, const int32_t *dims, const double *lo, const double *hi, int32_t n_params,
                                 int32_t device, void **out) {
  const char *who = "pcgrl_archive_create_genomes";
  if (out) *out = nullptr;
  if (n_params < 1 || n_params > EVO_MAX_PARAMS) return arch_fail(PCGRL_EINVAL, who, "the genome length must be in [1, 16384]");
  return arch_create(who, n_axes, dims, lo, hi, 4 * n_params, 0, device, out);
}

void pcgrl_archive_destroy(void *archive) {
  Archive *a = arch_of(archive);
  if (!a) return;
  a->tag = 0;
  (void)hipFree(a->block);
  delete a;
}

int pcgrl_archive_add(void *archive, int32_t n, const uint8_t *d_maps, const double *d_objectives, const double *d_behaviours,
                      const int32_t *d_cells, uint8_t *d_status, int32_t *d_cell, int32_t *d_counts, void *stream) {
  const char *who = "pcgrl_archive_add";
  Archive *a = arch_of(archive);
  if (!a) return arch_fail(PCGRL_EINVAL, who, "null or dead archive handle");
  if (n < 1) return arch_fail(PCGRL_EINVAL, who, "n must be at least 1");
  if (!d_maps || !d_objectives) return arch_fail(PCGRL_EINVAL, who, "d_maps and d_objectives must not be null");
  if (!d_behaviours && !d_cells) return arch_fail(PCGRL_EINVAL, who, "d_behaviours or d_cells is needed");
  if (!d_status || !d_cell || !d_counts) return arch_fail(PCGRL_EINVAL, who, "d_status, d_cell and d_counts must not be null");
  ArchAddArgs k;
  k.g = a->g, k.m = a->m, k.n = n, k.maps = d_maps, k.objectives = d_objectives, k.behaviours = d_behaviours, k.cells = d_cells;
  k.status = d_status, k.cell = d_cell, k.counts = d_counts;
  ARCH_HIPCHK(launch_arch_add(k, (hipStream_t)stream));
  ARCH_HIPCHK(launch_arch_scan(a->g, a->m, d_counts, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_archive_cells(void *archive, int32_t n, const double *d_behaviours, int32_t *d_cell, void *stream) {
  const char *who = "pcgrl_archive_cells";
  Archive *a = arch_of(archive);
  if (!a) return arch_fail(PCGRL_EINVAL, who, "null or dead archive handle");
  if (n < 1) return arch_fail(PCGRL_EINVAL, who, "n must be at least 1");
  if (!d_behaviours || !d_cell) return arch_fail(PCGRL_EINVAL, who, "d_behaviours and d_cell must not be null");
  ARCH_HIPCHK(launch_arch_cells(a->g, n, d_behaviours, d_cell, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_archive_stats(void *archive, double *d_stats, void *stream) {
  const char *who = "pcgrl_archive_stats";
  Archive *a = arch_of(archive);
  if (!a) return arch_fail(PCGRL_EINVAL, who, "null or dead archive handle");
  if (!d_stats) return arch_fail(PCGRL_EINVAL, who, "d_stats must not be null");
  ARCH_HIPCHK(launch_arch_stats(a->m, d_stats, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_archive_elites(void *archive, int32_t cap, int32_t *d_cells, double *d_objectives, double *d_behaviours,
                         uint8_t *d_maps, void *stream) {
  const char *who = "pcgrl_archive_elites";
  Archive *a = arch_of(archive);
  if (!a) return arch_fail(PCGRL_EINVAL, who, "null or dead archive handle");
  if (cap < 1) return arch_fail(PCGRL_EINVAL, who, "cap must be at least 1");
  ArchElitesArgs k;
  k.g = a->g, k.m = a->m, k.cap = cap < a->g.cells ? cap : a->g.cells, k.cells = d_cells, k.objectives = d_objectives;
  k.behaviours = d_behaviours, k.maps = d_maps;
  ARCH_HIPCHK(launch_arch_elites(k, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_archive_ask(void *archive, int32_t n, uint64_t seed, double rate, uint8_t *d_out_maps, int32_t *d_out_parent_cell,
                      void *stream) {
  const char *who = "pcgrl_archive_ask";
  Archive *a = arch_of(archive);
  if (!a) return arch_fail(PCGRL_EINVAL, who, "null or dead archive handle");
  if (n < 1) return arch_fail(PCGRL_EINVAL, who, "n must be at least 1");
  if (!(rate >= 0.0 && rate <= 1.0)) return arch_fail(PCGRL_EINVAL, who, "rate must be in [0, 1]");
  if (!d_out_maps) return arch_fail(PCGRL_EINVAL, who, "d_out_maps must not be null");
  if (a->g.T == 0) return arch_fail(PCGRL_EINVAL, who, "a genome archive has no tiles to flip: use pcgrl_archive_ask_genomes");
  ArchAskArgs k;
  k.g = a->g, k.m = a->m, k.n = n, k.seed = seed, k.rate = rate, k.out = d_out_maps, k.parent_cell = d_out_parent_cell;
  ARCH_HIPCHK(launch_arch_ask(k, (hipStream_t)stream));
  return PCGRL_OK;
}

int64_t pcgrl_archive_state_bytes(void *archive) {
  Archive *a = arch_of(archive);
  if (!a) {
    arch_fail(PCGRL_EINVAL, "pcgrl_archive_state_bytes", "null or dead archive handle");
    return -1;
  }
  return (int64_t)image_layout(a->g).total;
}

int pcgrl_archive_export(void *archive, void *d_image, void *stream) {
  const char *who = "pcgrl_archive_export";
  Archive *a = arch_of(archive);
  if (!a) return arch_fail(PCGRL_EINVAL, who, "null or dead archive handle");
  if (!d_image || ((uintptr_t)d_image & 15u)) return arch_fail(PCGRL_EINVAL, who, "d_image is null or not 16-byte aligned");
  const ArchGrid &g = a->g;
  const ImageLayout l = image_layout(g);
  hipStream_t s = (hipStream_t)stream;
  uint8_t *img = (uint8_t *)d_image;
  ARCH_HIPCHK(launch_arch_export_header(g, a->m, d_image, s));
  ARCH_HIPCHK(hipMemsetAsync(img + l.obj, 0, l.total - l.obj, s));  // (the padding of the sections)
  ARCH_HIPCHK(hipMemcpyAsync(img + l.obj, a->m.obj, (size_t)g.cells * 8, hipMemcpyDeviceToDevice, s));
  ARCH_HIPCHK(hipMemcpyAsync(img + l.beh, a->m.beh, (size_t)g.cells * g.D * 8, hipMemcpyDeviceToDevice, s));
  ARCH_HIPCHK(hipMemcpyAsync(img + l.maps, a->m.maps, (size_t)g.cells * g.LP, hipMemcpyDeviceToDevice, s));
  ARCH_HIPCHK(hipMemcpyAsync(img + l.flag, a->m.flag, (size_t)g.cells, hipMemcpyDeviceToDevice, s));
  return PCGRL_OK;
}

int pcgrl_archive_import(void *archive, const void *d_image, int64_t image_bytes, const void *h_header, void *stream) {
  const char *who = "pcgrl_archive_import";
  Archive *a = arch_of(archive);
  if (!a) return arch_fail(PCGRL_EINVAL, who, "null or dead archive handle");
  if (!d_image || ((uintptr_t)d_image & 15u)) return arch_fail(PCGRL_EINVAL, who, "d_image is null or not 16-byte aligned");
  if (!h_header) return arch_fail(PCGRL_EINVAL, who, "h_header must not be null");
  const ArchGrid &g = a->g;
  ArchHeader h;
  std::memcpy(&h, h_header, sizeof h);
  if (h.magic != ARCH_MAGIC) return arch_fail(PCGRL_EINVAL, who, "not an archive image");
  if (h.version != PCGRL_ARCHIVE_IMAGE_VERSION) return arch_fail(PCGRL_EINVAL, who, "an image of another version");
  if (h.D != g.D) return arch_fail(PCGRL_EINVAL, who, "the image has another number of behaviour axes");
  for (int j = 0; j < g.D; j++) {
    if (h.dims[j] != g.dims[j]) return arch_fail(PCGRL_EINVAL, who, "the image has other dims");
    if (h.lo[j] != g.lo[j] || h.hi[j] != g.hi[j]) return arch_fail(PCGRL_EINVAL, who, "the image has other bounds");
  }
  if ((h.T == 0) != (g.T == 0))
    return arch_fail(PCGRL_EINVAL, who, g.T == 0 ? "a map archive's image does not fit a genome archive"
                                                 : "a genome archive's image does not fit a map archive");
  if (h.L != g.L) return arch_fail(PCGRL_EINVAL, who, g.T == 0 ? "the image has another genome length" : "the image has another map length");
  if (h.T != g.T) return arch_fail(PCGRL_EINVAL, who, "the image has another tile count");
  const ImageLayout l = image_layout(g);
  if (image_bytes != (int64_t)l.total) return arch_fail(PCGRL_EINVAL, who, "the image has another size");
  hipStream_t s = (hipStream_t)stream;
  const uint8_t *img = (const uint8_t *)d_image;
  ARCH_HIPCHK(hipMemcpyAsync(a->m.obj, img + l.obj, (size_t)g.cells * 8, hipMemcpyDeviceToDevice, s));
  ARCH_HIPCHK(hipMemcpyAsync(a->m.beh, img + l.beh, (size_t)g.cells * g.D * 8, hipMemcpyDeviceToDevice, s));
  ARCH_HIPCHK(hipMemcpyAsync(a->m.maps, img + l.maps, (size_t)g.cells * g.LP, hipMemcpyDeviceToDevice, s));
  ARCH_HIPCHK(hipMemcpyAsync(a->m.flag, img + l.flag, (size_t)g.cells, hipMemcpyDeviceToDevice, s));
  ARCH_HIPCHK(launch_arch_import_finish(g, a->m, d_image, s));
  ARCH_HIPCHK(launch_arch_scan(g, a->m, nullptr, s));
  return PCGRL_OK;
}

int pcgrl_archive_poll_error(void *archive, void *stream) {
  Archive *a = arch_of(archive);
  if (!a) {
    arch_fail(PCGRL_EINVAL, "pcgrl_archive_poll_error", "null or dead archive handle");
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  uint32_t bits = 0;
  hipError_t e = hipMemcpyAsync(&bits, a->m.error, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipMemsetAsync(a->m.error, 0, 4, s);
  if (e != hipSuccess) {
    arch_fail(PCGRL_EHIP, "pcgrl_archive_poll_error", hipGetErrorString(e));
    return -1;
  }
  return (int)bits;
}

static int evo_children(const char *who, int with_parent, void *archive, int32_t n, uint64_t seed, float sigma, const float *d_mean,
                        float *d_out, int32_t *d_out_parent_cell, void *stream) {
  Archive *a = arch_of(archive);
  if (!a) return arch_fail(PCGRL_EINVAL, who, "null or dead archive handle");
  if (n < 1) return arch_fail(PCGRL_EINVAL, who, "n must be at least 1");
  if (!(sigma >= 0.0f) || !std::isfinite(sigma)) return arch_fail(PCGRL_EINVAL, who, "sigma must be finite and not negative");
  if (!d_out || ((uintptr_t)d_out & 3u)) return arch_fail(PCGRL_EINVAL, who, "d_out is null or not 4-byte aligned");
  if (d_mean && ((uintptr_t)d_mean & 3u)) return arch_fail(PCGRL_EINVAL, who, "d_mean is not 4-byte aligned");
  if (a->g.T != 0)
    return arch_fail(PCGRL_EINVAL, who, "a map archive holds no genomes: use pcgrl_archive_ask (pcgrl_archive_create_genomes "
                                        "makes a genome archive)");
  EvoChildrenArgs k;
  k.g = a->g, k.m = a->m, k.n = n, k.P = a->g.L / 4, k.with_parent = with_parent, k.seed = seed, k.sigma = sigma, k.mean = d_mean;
  k.out = d_out, k.parent_cell = d_out_parent_cell;
  ARCH_HIPCHK(launch_evo_children(k, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_archive_ask_genomes(void *archive, int32_t n, uint64_t seed, float sigma, float *d_out, int32_t *d_out_parent_cell,
                              void *stream) {
  return evo_children("pcgrl_archive_ask_genomes", 1, archive, n, seed, sigma, nullptr, d_out, d_out_parent_cell, stream);
}

int pcgrl_archive_sample_genomes(void *archive, int32_t n, uint64_t seed, float sigma, const float *d_mean, float *d_out,
                                 void *stream) {
  return evo_children("pcgrl_archive_sample_genomes", 0, archive, n, seed, sigma, d_mean, d_out, nullptr, stream);
}

int pcgrl_evo_aggregate(int32_t n_genomes, int32_t n_seeds, int32_t n_behaviours, double weight, const double *d_objective,
                        const double *d_behaviours, const int32_t *d_n_step, double *d_out_behaviours, double *d_out_objective,
                        int32_t *d_out_time_penalty, double *d_out_variance_penalty, uint8_t *d_out_valid, void *stream) {
  const char *who = "pcgrl_evo_aggregate";
  if (n_genomes < 1) return arch_fail(PCGRL_EINVAL, who, "the number of genomes must be at least 1");
  if (n_seeds < 1 || n_seeds > EVO_MAX_SEEDS) return arch_fail(PCGRL_EINVAL, who, "the number of seeds must be in [1, 128]");
  if (n_behaviours < 1 || n_behaviours > EVO_MAX_BEHAVIOURS)
    return arch_fail(PCGRL_EINVAL, who, "the number of behaviours must be in [1, 4]");
  if (!d_objective || !d_behaviours || !d_n_step) return arch_fail(PCGRL_EINVAL, who, "the inputs must not be null");
  if (!d_out_behaviours || !d_out_objective || !d_out_time_penalty || !d_out_variance_penalty || !d_out_valid)
    return arch_fail(PCGRL_EINVAL, who, "the outputs must not be null");
  EvoAggregateArgs k;
  k.G = n_genomes, k.S = n_seeds, k.D = n_behaviours, k.weight = weight, k.objective = d_objective, k.behaviours = d_behaviours;
  k.n_step = d_n_step, k.out_behaviours = d_out_behaviours, k.out_objective = d_out_objective, k.out_time = d_out_time_penalty;
  k.out_variance = d_out_variance_penalty, k.out_valid = d_out_valid;
  ARCH_HIPCHK(launch_evo_aggregate(k, (hipStream_t)stream));
  return PCGRL_OK;
}

}  // extern "C"
