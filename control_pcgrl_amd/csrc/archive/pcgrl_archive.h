// archive/pcgrl_archive.h -- the quality-diversity grid archive on the device (include/pcgrl_amd_archive.h): placement,
// batch insertion, the occupied list and its statistics, parent selection and mutation, the image.  DESIGN.md section 35 has
// the rules; tests/archive_rules.py is the same, one candidate at a time, in numpy.
//
// Per cell in HBM: obj double, beh double [D], flag uint8, the map in a row of LP = L rounded up to 16 bytes (so a row starts
// 16-byte aligned and is written with 16-byte stores; the bytes past L are zero), and two scratch words:
//   word  uint64  the order-preserving key of the occupant's objective, 0 when the cell is empty (no double has key 0)
//   win   int32   INT32_MAX
// Both hold between calls, so an add seeds nothing: the key pass raises `word`, the commit pass puts `win` back.
//
// A genome archive (include/pcgrl_amd_evo.h, evo/pcgrl_evo.h) is the same archive with T = 0 and a row of L = 4 P bytes, the P
// float32 weights of an NCA genome (L up to 65536): every kernel below copies a row as bytes and serves it unchanged; only
// arch_ask_kernel, which flips tiles, is refused for it on the host.
//
// pcgrl_archive_add, kernels on one stream (a kernel boundary is the only barrier):
//   arch_key_kernel     thread per candidate: its cell (placement, or the caller's index) into the caller's d_cell, -1 and
//                       status 3 and error bit 0 when refused; 64-bit atomicMax of its key into word[cell]
//   arch_winner_kernel  thread per candidate: when its key equals word[cell] and exceeds the occupant's (obj[cell] is still
//                       the occupant's), 32-bit atomicMin of its batch index into win[cell]
//   arch_status_kernel  thread per candidate: status from win[cell] and flag[cell]; counts by wave ballot, one atomic per wave
//                       and counter
//   arch_commit_kernel  wave per candidate: the winner copies its map (lane j the 16 bytes at 16 j; 16-byte loads when the
//                       caller's rows are 16-byte aligned, else byte loads; always 16-byte stores), lane 0 writes obj, beh,
//                       flag and puts win[cell] back
//   arch_scan_kernel    one block of 1024 threads: thread t owns the cells [t * chunk, (t + 1) * chunk); counts, a scan by wave
//                       shuffles and one LDS exchange of the sixteen wave totals, then the occupied list in ascending order,
//                       the count, max, min and the sum (a thread's cells in ascending order, a fixed butterfly over the
//                       wave, the waves in ascending order)
// Integer max / min atomics commute, so the result does not depend on arrival order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcgrl {

constexpr int ARCH_MAX_AXES = 4;
constexpr int ARCH_MAX_CELLS = 1 << 20;
constexpr int ARCH_MAX_L = 4096;
constexpr int ARCH_MAX_T = 256;
constexpr int ARCH_SCAN_THREADS = 1024;
constexpr int32_t ARCH_NO_WINNER = 0x7FFFFFFF;
constexpr uint32_t ARCH_MAGIC = 0x41514350u;  // "PCQA"
constexpr int ARCH_HEADER_BYTES = 128;

struct ArchGrid {
  int32_t D, cells, L, LP, T;
  int32_t dims[ARCH_MAX_AXES];
  double lo[ARCH_MAX_AXES], hi[ARCH_MAX_AXES];
};

// device pointers of one archive
struct ArchMem {
  double *obj;        // [cells]
  double *beh;        // [cells][D]
  uint8_t *flag;      // [cells]
  uint8_t *maps;      // [cells][LP]
  uint64_t *word;     // [cells]
  int32_t *win;       // [cells]
  int32_t *occ;       // [cells]: the occupied cells in ascending order, the first stats_i[0] entries
  int32_t *stats_i;   // [1]: the occupied count
  double *stats_d;    // [3]: max, min, sum
  uint64_t *draw;     // [1]
  uint32_t *error;    // [1]
};

struct ArchAddArgs {
  ArchGrid g;
  ArchMem m;
  int32_t n;
  const uint8_t *maps;
  const double *objectives, *behaviours;  // behaviours may be null when cells is given
  const int32_t *cells;                   // or null
  uint8_t *status;
  int32_t *cell;
  int32_t *counts;
};

struct ArchAskArgs {
  ArchGrid g;
  ArchMem m;
  int32_t n;
  uint64_t seed;
  double rate;
  uint8_t *out;
  int32_t *parent_cell;  // or null
};

struct ArchElitesArgs {
  ArchGrid g;
  ArchMem m;
  int32_t cap;
  int32_t *cells;
  double *objectives, *behaviours;
  uint8_t *maps;
};

__host__ __device__ inline uint64_t arch_mix64(uint64_t z) {  // splitmix64 finaliser (trg_mix64 of pcgrl_kernels2d.h)
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__host__ __device__ inline double arch_u01(uint64_t z) { return (double)(z >> 11) * (1.0 / 9007199254740992.0); }

hipError_t launch_arch_add(const ArchAddArgs &a, hipStream_t s);
hipError_t launch_arch_cells(const ArchGrid &g, int32_t n, const double *beh, int32_t *cell, hipStream_t s);
hipError_t launch_arch_scan(const ArchGrid &g, const ArchMem &m, int32_t *counts, hipStream_t s);
hipError_t launch_arch_stats(const ArchMem &m, double *out, hipStream_t s);
hipError_t launch_arch_elites(const ArchElitesArgs &a, hipStream_t s);
hipError_t launch_arch_ask(const ArchAskArgs &a, hipStream_t s);
hipError_t launch_arch_clear(const ArchGrid &g, const ArchMem &m, hipStream_t s);
hipError_t launch_arch_export_header(const ArchGrid &g, const ArchMem &m, void *image, hipStream_t s);
hipError_t launch_arch_import_finish(const ArchGrid &g, const ArchMem &m, const void *image, hipStream_t s);

#ifdef PCGRL_ARCHIVE_KERNEL  // (archive/pcgrl_k_archive.hip has it)

// An order-preserving 64-bit image of a double that is not NaN: -0.0 is folded onto 0.0 first (x + 0.0), a negative value has
// all its bits flipped and any other its sign bit set.  -inf maps to 0x000fffffffffffff, so no value maps to 0.
__device__ __forceinline__ uint64_t arch_key(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x + 0.0);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the cell of one behaviour vector, -1 with a NaN in it
__device__ __forceinline__ int32_t arch_place(const ArchGrid &g, const double *x) {
  int32_t cell = 0;
  for (int j = 0; j < g.D; j++) {
    const double v = x[j], lo = g.lo[j], hi = g.hi[j];
    if (v != v) return -1;
    double b = v < lo ? lo : v;
    b = b > hi ? hi : b;
    int32_t i = (int32_t)(((b - lo) / (hi - lo)) * (double)g.dims[j]);
    i = i < g.dims[j] - 1 ? i : g.dims[j] - 1;
    cell = cell * g.dims[j] + i;
  }
  return cell;
}

__global__ __launch_bounds__(256) void arch_cells_kernel(const ArchGrid g, int32_t n, const double *beh, int32_t *cell) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) cell[i] = arch_place(g, beh + (size_t)i * g.D);
}

__global__ __launch_bounds__(256) void arch_key_kernel(const ArchAddArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) a.counts[0] = a.counts[1] = a.counts[2] = a.counts[3] = 0;
  if (i >= a.n) return;
  const double o = a.objectives[i];
  int32_t cell;
  if (a.cells) {
    cell = a.cells[i];
    if (cell < 0 || cell >= a.g.cells) cell = -1;
    if (a.behaviours)
      for (int j = 0; j < a.g.D; j++) {
        const double v = a.behaviours[(size_t)i * a.g.D + j];
        if (v != v) cell = -1;
      }
  } else {
    cell = arch_place(a.g, a.behaviours + (size_t)i * a.g.D);
  }
  if (o != o) cell = -1;
  a.cell[i] = cell;
  if (cell < 0) {
    a.status[i] = 3;
    atomicOr(a.m.error, 1u);
    return;
  }
  atomicMax((unsigned long long *)&a.m.word[cell], (unsigned long long)arch_key(o));
}

__global__ __launch_bounds__(256) void arch_winner_kernel(const ArchAddArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int32_t cell = a.cell[i];
  if (cell < 0) return;
  const uint64_t key = arch_key(a.objectives[i]);
  const uint64_t okey = a.m.flag[cell] ? arch_key(a.m.obj[cell]) : 0ull;
  if (key == a.m.word[cell] && key > okey) atomicMin(&a.m.win[cell], i);
}

__global__ __launch_bounds__(256) void arch_status_kernel(const ArchAddArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int st = 0;
  bool refused = false;
  if (i < a.n) {
    const int32_t cell = a.cell[i];
    if (cell < 0) {
      refused = true;
    } else {
      if (a.m.win[cell] == i) st = a.m.flag[cell] ? 1 : 2;
      a.status[i] = (uint8_t)st;
    }
  }
  const int n_new = __popcll(__ballot(st == 2)), n_imp = __popcll(__ballot(st == 1)), n_ref = __popcll(__ballot(refused));
  if ((threadIdx.x & 63) == 0) {
    if (n_new) atomicAdd(&a.counts[0], n_new);
    if (n_imp) atomicAdd(&a.counts[1], n_imp);
    if (n_ref) atomicAdd(&a.counts[2], n_ref);
  }
}

// 256 threads = 4 waves = 4 candidates
__global__ __launch_bounds__(256) void arch_commit_kernel(const ArchAddArgs a) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= a.n) return;
  const uint8_t st = a.status[i];
  if (st != 1 && st != 2) return;
  const int32_t cell = a.cell[i];
  const int L = a.g.L, LP = a.g.LP;
  const uint8_t *src = a.maps + (size_t)i * L;
  uint8_t *dst = a.m.maps + (size_t)cell * LP;
  const bool aligned = (((uintptr_t)a.maps | (uintptr_t)L) & 15u) == 0;  // every caller row starts 16-byte aligned and LP == L
  for (int off = lane * 16; off < LP; off += 64 * 16) {
    uint4 v;
    if (aligned) {
      v = *(const uint4 *)(src + off);
    } else {
      uint32_t w[4] = {0, 0, 0, 0};
      for (int k = 0; k < 16; k++)
        if (off + k < L) w[k >> 2] |= (uint32_t)src[off + k] << (8 * (k & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *(uint4 *)(dst + off) = v;
  }
  if (lane == 0) {
    a.m.obj[cell] = a.objectives[i];
    for (int j = 0; j < a.g.D; j++) a.m.beh[(size_t)cell * a.g.D + j] = a.behaviours ? a.behaviours[(size_t)i * a.g.D + j] : 0.0;
    a.m.flag[cell] = 1;
    a.m.win[cell] = ARCH_NO_WINNER;
  }
}

// One block.  counts (may be null): the fourth entry gets the occupied count.
__global__ __launch_bounds__(ARCH_SCAN_THREADS) void arch_scan_kernel(const ArchGrid g, const ArchMem m, int32_t *counts) {
  constexpr int WAVES = ARCH_SCAN_THREADS / 64;
  __shared__ int32_t s_cnt[WAVES];
  __shared__ double s_max[WAVES], s_min[WAVES], s_sum[WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int chunk = (g.cells + ARCH_SCAN_THREADS - 1) / ARCH_SCAN_THREADS;
  const int c0 = min(t * chunk, g.cells), c1 = min(c0 + chunk, g.cells);
  int cnt = 0;
  double mx = -__builtin_inf(), mn = __builtin_inf(), sum = 0.0;
  // eight cells at a time: the sixteen loads of a round do not depend on one another (the index is clamped, the value masked)
  for (int c = c0; c < c1; c += 8) {
    uint8_t f[8];
    double o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int at = min(c + k, g.cells - 1);
      f[k] = m.flag[at];
      o[k] = m.obj[at];
    }
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (c + k < c1 && f[k]) {
        cnt++;
        mx = o[k] > mx ? o[k] : mx;
        mn = o[k] < mn ? o[k] : mn;
        sum += o[k];
      }
  }
  // inside the wave: an inclusive scan of the counts, and max, min and sum over a fixed butterfly (a + b is b + a, so every
  // lane ends with the same bits)
  int inc = cnt;
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(inc, d, 64);
    if (lane >= d) inc += v;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const double omx = __shfl_xor(mx, d, 64), omn = __shfl_xor(mn, d, 64), osum = __shfl_xor(sum, d, 64);
    mx = omx > mx ? omx : mx;
    mn = omn < mn ? omn : mn;
    sum = sum + osum;
  }
  if (lane == 63) s_cnt[wave] = inc;
  if (lane == 0) s_max[wave] = mx, s_min[wave] = mn, s_sum[wave] = sum;
  __syncthreads();
  int at = inc - cnt;
  for (int w = 0; w < wave; w++) at += s_cnt[w];
  for (int c = c0; c < c1; c += 8) {
    uint8_t f[8];
#pragma unroll
    for (int k = 0; k < 8; k++) f[k] = m.flag[min(c + k, g.cells - 1)];
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (c + k < c1 && f[k]) m.occ[at++] = c + k;
  }
  if (t == 0) {  // the waves in ascending order
    int total = 0;
    double tmx = s_max[0], tmn = s_min[0], tsum = s_sum[0];
    for (int w = 0; w < WAVES; w++) total += s_cnt[w];
    for (int w = 1; w < WAVES; w++) {
      tmx = s_max[w] > tmx ? s_max[w] : tmx;
      tmn = s_min[w] < tmn ? s_min[w] : tmn;
      tsum = tsum + s_sum[w];
    }
    m.stats_i[0] = total;
    m.stats_d[0] = tmx, m.stats_d[1] = tmn, m.stats_d[2] = tsum;
    if (counts) counts[3] = total;
  }
}

__global__ void arch_stats_kernel(const ArchMem m, double *out) {
  if (threadIdx.x == 0) {
    out[0] = (double)m.stats_i[0];
    out[1] = m.stats_d[0], out[2] = m.stats_d[1], out[3] = m.stats_d[2];
  }
}

// thread per (elite, map byte); the thread of byte 0 writes the elite's cell, objective and behaviours
__global__ __launch_bounds__(256) void arch_elites_kernel(const ArchElitesArgs a) {
  const int count = min(a.m.stats_i[0], a.cap);
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int e = (int)(idx / a.g.L), k = (int)(idx % a.g.L);
  if (e >= count) return;
  const int32_t cell = a.m.occ[e];
  if (a.maps) a.maps[(size_t)e * a.g.L + k] = a.m.maps[(size_t)cell * a.g.LP + k];
  if (k == 0) {
    if (a.cells) a.cells[e] = cell;
    if (a.objectives) a.objectives[e] = a.m.obj[cell];
    if (a.behaviours)
      for (int j = 0; j < a.g.D; j++) a.behaviours[(size_t)e * a.g.D + j] = a.m.beh[(size_t)cell * a.g.D + j];
  }
}

// a row of blocks per child (blockIdx.x the child, blockIdx.y the block of bytes), thread per byte: what depends on the child alone is uniform over the block
__global__ __launch_bounds__(256) void arch_ask_kernel(const ArchAskArgs a) {
  const int count = a.m.stats_i[0];
  const int c = blockIdx.x, k = blockIdx.y * blockDim.x + threadIdx.x;
  if (count <= 0) {
    if (c == 0 && k == 0) atomicOr(a.m.error, 2u);
    return;
  }
  if (c >= a.n || k >= a.g.L) return;
  const uint64_t base = arch_mix64(a.seed + a.m.draw[0] * 0x9e3779b97f4a7c15ull);
  const uint64_t cw = (uint64_t)(uint32_t)c * 0xd1b54a32d192ed03ull;
  int p = (int)(arch_u01(arch_mix64(base ^ (cw + 0x8cb92ba72f3d8dd7ull))) * (double)count);
  p = p < count - 1 ? p : count - 1;  // (u < 1, so this holds already)
  const int32_t cell = a.m.occ[p];
  uint32_t t = a.m.maps[(size_t)cell * a.g.LP + k];
  if (a.g.T > 1) {
    const uint64_t cb = arch_mix64(base ^ (cw + 2ull * 0x8cb92ba72f3d8dd7ull));
    const uint64_t q = arch_mix64(cb + (uint64_t)(k + 1) * 0x9e3779b97f4a7c15ull);
    if (arch_u01(q) < a.rate) {
      const int r = (int)(arch_u01(arch_mix64(q ^ 0x8cb92ba72f3d8dd7ull)) * (double)(a.g.T - 1));
      t = (t + 1u + (uint32_t)r) % (uint32_t)a.g.T;
    }
  }
  a.out[(size_t)c * a.g.L + k] = (uint8_t)t;
  if (k == 0 && a.parent_cell) a.parent_cell[c] = cell;
}

// after every thread of arch_ask_kernel has read the counter
__global__ void arch_bump_kernel(const ArchMem m) {
  if (threadIdx.x == 0 && m.stats_i[0] > 0) m.draw[0] += 1;
}

// an empty archive (create)
__global__ __launch_bounds__(256) void arch_clear_kernel(const ArchGrid g, const ArchMem m) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c == 0) m.draw[0] = 0, m.error[0] = 0;
  if (c >= g.cells) return;
  m.obj[c] = 0.0;
  for (int j = 0; j < g.D; j++) m.beh[(size_t)c * g.D + j] = 0.0;
  m.flag[c] = 0;
  m.word[c] = 0;
  m.win[c] = ARCH_NO_WINNER;
  for (int k = 0; k < g.LP; k += 16) *(uint4 *)(m.maps + (size_t)c * g.LP + k) = make_uint4(0, 0, 0, 0);
}

struct ArchHeader {  // PCGRL_ARCHIVE_HEADER_BYTES
  uint32_t magic;
  int32_t version, D, dims[ARCH_MAX_AXES], L, T, zero;
  double lo[ARCH_MAX_AXES], hi[ARCH_MAX_AXES];
  uint64_t draw;
  uint64_t pad[2];
};
static_assert(sizeof(ArchHeader) == ARCH_HEADER_BYTES, "the image header is 128 bytes");

__global__ void arch_export_header_kernel(const ArchGrid g, const ArchMem m, ArchHeader *h) {
  if (threadIdx.x != 0) return;
  h->magic = ARCH_MAGIC, h->version = 1, h->D = g.D, h->L = g.L, h->T = g.T, h->zero = 0;
  for (int j = 0; j < ARCH_MAX_AXES; j++) {
    h->dims[j] = j < g.D ? g.dims[j] : 0;
    h->lo[j] = j < g.D ? g.lo[j] : 0.0;
    h->hi[j] = j < g.D ? g.hi[j] : 0.0;
  }
  h->draw = m.draw[0];
  h->pad[0] = h->pad[1] = 0;
}

// after the sections of an image are in place: the draw counter, and the scratch words from the objectives and the flags
__global__ __launch_bounds__(256) void arch_import_finish_kernel(const ArchGrid g, const ArchMem m, const ArchHeader *h) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c == 0) m.draw[0] = h->draw;
  if (c >= g.cells) return;
  const bool occ = m.flag[c] != 0;
  m.flag[c] = occ ? 1 : 0;
  m.word[c] = occ ? arch_key(m.obj[c]) : 0ull;
  m.win[c] = ARCH_NO_WINNER;
}

#endif  // PCGRL_ARCHIVE_KERNEL

}  // namespace pcgrl
