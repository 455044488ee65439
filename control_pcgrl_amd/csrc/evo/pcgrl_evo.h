// evo/pcgrl_evo.h -- NCA evolution on the device (include/pcgrl_amd_evo.h): the normal draw with stated arithmetic, the
// Gaussian children of a genome archive, and simulate's fold over seeds.  DESIGN.md section 42 has the rules;
// control_pcgrl_amd/evo.py has the numpy twins (log64, normal_from_uniform, gaussian_children, aggregated) that these kernels
// equal bit for bit.
//
// A genome archive is the grid archive of archive/pcgrl_archive.h with a payload row of L = 4 P bytes (P float32 values) and
// T = 0 where a map archive has its tile count: placement, insertion, the occupied list, the statistics and the image are the
// same kernels on the same rows, so the insertion is written once.  This header is included by archive/pcgrl_k_archive.hip,
// which owns the handle.
//
//   evo_children_kernel   a row of blocks per child (blockIdx.x the child, blockIdx.y the block of 1024 elements), four elements
//                         per thread: the parent draw is uniform over the block; per element one 4-byte load, two mixes, ppnd
//                         in float64 (the tails compacted through LDS onto full waves), one float32 multiply, one float32 add,
//                         one 4-byte store (a wave stores 256 contiguous bytes)
//   evo_aggregate_kernel  thread per genome: the S values of a genome are summed in numpy's order, every load explicit
//
// Only + - * /, correctly rounded sqrt, comparisons and bit operations; no fused multiply-add.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../archive/pcgrl_archive.h"

namespace pcgrl {

constexpr int EVO_MAX_PARAMS = 16384;
constexpr int EVO_MAX_SEEDS = 128;
constexpr int EVO_MAX_BEHAVIOURS = 4;

struct EvoChildrenArgs {
  ArchGrid g;
  ArchMem m;
  int32_t n, P;
  int32_t with_parent;  // 1: ask_genomes, 0: sample_genomes
  uint64_t seed;
  float sigma;
  const float *mean;     // sample_genomes: [P] or null
  float *out;            // [n][P]
  int32_t *parent_cell;  // or null
};

struct EvoAggregateArgs {
  int32_t G, S, D;
  double weight;
  const double *objective;   // [G][S]
  const double *behaviours;  // [G][S][D]
  const int32_t *n_step;     // [G][S]
  double *out_behaviours;    // [G][D]
  double *out_objective;     // [G]
  int32_t *out_time;         // [G]
  double *out_variance;      // [G]
  uint8_t *out_valid;        // [G]
};

hipError_t launch_evo_children(const EvoChildrenArgs &a, hipStream_t s);
hipError_t launch_evo_aggregate(const EvoAggregateArgs &a, hipStream_t s);

#ifdef PCGRL_ARCHIVE_KERNEL

#pragma clang fp contract(off)  // every multiply and every add is rounded on its own

// This project's float64 natural logarithm of a positive normal x: x = m 2^e by the bits with m in [sqrt(1/2), sqrt(2)),
// f = (m - 1) / (m + 1), p the Horner polynomial in f^2 with the coefficients 1/25, 1/23, ..., 1/1, and
// e ln2_hi + ((2 f) p + e ln2_lo).
__host__ __device__ inline double evo_log64(double x) {
  union {
    double d;
    uint64_t b;
  } v;
  v.d = x;
  int e = (int)((v.b >> 52) & 0x7ffu) - 1022;
  v.b = (v.b & 0x000fffffffffffffull) | 0x3fe0000000000000ull;  // [1/2, 1)
  double m = v.d;
  if (m < 0.70710678118654757) {
    m = m * 2.0;
    e -= 1;
  }
  const double f = (m - 1.0) / (m + 1.0);
  const double s = f * f;
  double p = 1.0 / 25.0;
  p = p * s + 1.0 / 23.0;
  p = p * s + 1.0 / 21.0;
  p = p * s + 1.0 / 19.0;
  p = p * s + 1.0 / 17.0;
  p = p * s + 1.0 / 15.0;
  p = p * s + 1.0 / 13.0;
  p = p * s + 1.0 / 11.0;
  p = p * s + 1.0 / 9.0;
  p = p * s + 1.0 / 7.0;
  p = p * s + 1.0 / 5.0;
  p = p * s + 1.0 / 3.0;
  p = p * s + 1.0;
  const double de = (double)e;
  return de * 6.93147180369123816490e-01 + ((2.0 * f) * p + de * 1.90821492927058770002e-10);
}

__host__ __device__ inline double evo_sqrt64(double x) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dsqrt_rn(x);
#else
  return __builtin_sqrt(x);
#endif
}

// Wichura's AS241 PPND16 at 0 < u < 1: numerator and denominator by Horner, one division.  The central region
// (|u - 0.5| <= 0.425, 85 % of the draws) and the tails are functions of their own: the kernel runs them in separate passes.
__host__ __device__ inline bool evo_ppnd_is_central(double u) {
  const double q = u - 0.5;
  return (q < 0.0 ? -q : q) <= 0.425;
}

__host__ __device__ inline double evo_ppnd_central(double u) {
  const double q = u - 0.5;
  {
    const double r = 0.180625 - q * q;
    double num = 2.5090809287301226727e+3;
    num = num * r + 3.3430575583588128105e+4;
    num = num * r + 6.7265770927008700853e+4;
    num = num * r + 4.5921953931549871457e+4;
    num = num * r + 1.3731693765509461125e+4;
    num = num * r + 1.9715909503065514427e+3;
    num = num * r + 1.3314166789178437745e+2;
    num = num * r + 3.3871328727963666080e+0;
    num = num * q;
    double den = 5.2264952788528545610e+3;
    den = den * r + 2.8729085735721942674e+4;
    den = den * r + 3.9307895800092710610e+4;
    den = den * r + 2.1213794301586595867e+4;
    den = den * r + 5.3941960214247511077e+3;
    den = den * r + 6.8718700749205790830e+2;
    den = den * r + 4.2313330701600911252e+1;
    den = den * r + 1.0;
    return num / den;
  }
}

__host__ __device__ inline double evo_ppnd_tail(double u) {
  const double q = u - 0.5;
  const double t = q <= 0.0 ? u : 1.0 - u;  // min(u, 1 - u)
  double r = evo_sqrt64(-evo_log64(t));
  double num, den;
  if (r <= 5.0) {
    r = r - 1.6;
    num = 7.74545014278341407640e-4;
    num = num * r + 2.27238449892691845833e-2;
    num = num * r + 2.41780725177450611770e-1;
    num = num * r + 1.27045825245236838258e+0;
    num = num * r + 3.64784832476320460504e+0;
    num = num * r + 5.76949722146069140550e+0;
    num = num * r + 4.63033784615654529590e+0;
    num = num * r + 1.42343711074968357734e+0;
    den = 1.05075007164441684324e-9;
    den = den * r + 5.47593808499534494600e-4;
    den = den * r + 1.51986665636164571966e-2;
    den = den * r + 1.48103976427480074590e-1;
    den = den * r + 6.89767334985100004550e-1;
    den = den * r + 1.67638483018380384940e+0;
    den = den * r + 2.05319162663775882187e+0;
    den = den * r + 1.0;
  } else {
    r = r - 5.0;
    num = 2.01033439929228813265e-7;
    num = num * r + 2.71155556874348757815e-5;
    num = num * r + 1.24266094738807843860e-3;
    num = num * r + 2.65321895265761230930e-2;
    num = num * r + 2.96560571828504891230e-1;
    num = num * r + 1.78482653991729133580e+0;
    num = num * r + 5.46378491116411436990e+0;
    num = num * r + 6.65790464350110377720e+0;
    den = 2.04426310338993978564e-15;
    den = den * r + 1.42151175831644588870e-7;
    den = den * r + 1.84631831751005468180e-5;
    den = den * r + 7.86869131145613259100e-4;
    den = den * r + 1.48753612908506148525e-2;
    den = den * r + 1.36929880922735805310e-1;
    den = den * r + 5.99832206555888793770e-1;
    den = den * r + 1.0;
  }
  const double x = num / den;
  return q < 0.0 ? -x : x;
}

__host__ __device__ inline double evo_ppnd(double u) { return evo_ppnd_is_central(u) ? evo_ppnd_central(u) : evo_ppnd_tail(u); }

// u = ((q >> 11) + 0.5) 2^-53: never 0 or 1 ((q >> 11) + 0.5 is exact below 2^53)
__host__ __device__ inline double evo_u_open(uint64_t q) { return ((double)(q >> 11) + 0.5) * (1.0 / 9007199254740992.0); }

// EVO_EPT elements per thread, element j of thread t at k = block start + j * blockDim + t (a wave loads and stores 256 contiguous
// bytes).  Pass 1: the uniform and, in the central region, the draw; a tail uniform goes to a list in LDS.  Pass 2: the threads
// take the list's entries side by side, so the tail's logarithm, square root and second division run on full waves for the
// 15 % of the elements that need them and not, under a mask, for every element.  Pass 3: the child.  The order of the list
// does not matter: an entry carries its slot.
constexpr int EVO_EPT = 4;
constexpr int EVO_BLOCK = 256;

__global__ __launch_bounds__(EVO_BLOCK) void evo_children_kernel(const EvoChildrenArgs a) {
  __shared__ double s_u[EVO_BLOCK * EVO_EPT];
  __shared__ float s_z[EVO_BLOCK * EVO_EPT];
  __shared__ uint16_t s_slot[EVO_BLOCK * EVO_EPT];
  __shared__ int s_n;
  const int B = blockDim.x, t = threadIdx.x, c = blockIdx.x, k0 = blockIdx.y * (B * EVO_EPT) + t;
  int32_t cell = -1;
  const uint64_t base = arch_mix64(a.seed + a.m.draw[0] * 0x9e3779b97f4a7c15ull);
  const uint64_t cw = (uint64_t)(uint32_t)c * 0xd1b54a32d192ed03ull;
  if (a.with_parent) {  // (uniform over the block: no barrier has been reached)
    const int count = a.m.stats_i[0];
    if (count <= 0) {
      if (c == 0 && k0 == 0) atomicOr(a.m.error, 2u);
      return;
    }
    int p = (int)(arch_u01(arch_mix64(base ^ (cw + 0x8cb92ba72f3d8dd7ull))) * (double)count);
    p = p < count - 1 ? p : count - 1;
    cell = a.m.occ[p];
  }
  const float *row = a.with_parent ? (const float *)(a.m.maps + (size_t)cell * a.g.LP) : a.mean;
  if (t == 0) s_n = 0;
  __syncthreads();
  const uint64_t gb = arch_mix64(base ^ (cw + 3ull * 0x8cb92ba72f3d8dd7ull));
  float w[EVO_EPT], z[EVO_EPT];
  uint32_t tail = 0;
#pragma unroll
  for (int j = 0; j < EVO_EPT; j++) {
    const int k = k0 + j * B;
    w[j] = 0.0f, z[j] = 0.0f;
    if (k < a.P) {
      if (row) w[j] = row[k];
      const double u = evo_u_open(arch_mix64(gb + (uint64_t)(k + 1) * 0x9e3779b97f4a7c15ull));
      if (evo_ppnd_is_central(u)) {
        z[j] = (float)evo_ppnd_central(u);
      } else {
        const int i = atomicAdd(&s_n, 1);  // below EVO_BLOCK * EVO_EPT: one entry per element at most
        s_u[i] = u;
        s_slot[i] = (uint16_t)(j * B + t);
        tail |= 1u << j;
      }
    }
  }
  __syncthreads();
  const int n_tail = s_n;
  for (int i = t; i < n_tail; i += B) s_z[s_slot[i]] = (float)evo_ppnd_tail(s_u[i]);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < EVO_EPT; j++) {
    const int k = k0 + j * B;
    if (k < a.P) {
      const float zz = (tail >> j) & 1u ? s_z[j * B + t] : z[j];
      const float step = zz * a.sigma;
      a.out[(size_t)c * a.P + k] = a.sigma == 0.0f ? w[j] : w[j] + step;  // (sigma == 0 keeps a -0.0 weight's sign)
    }
  }
  if (k0 == 0 && a.parent_cell) a.parent_cell[c] = cell;
}

// after every thread of evo_children_kernel has read the counter; ask_genomes on an empty archive drew nothing
__global__ void evo_bump_kernel(const ArchMem m, int32_t with_parent) {
  if (threadIdx.x == 0 && (!with_parent || m.stats_i[0] > 0)) m.draw[0] += 1;
}

// numpy's sum of n doubles x[0], x[stride], ...: sequential below 8; from 8 to 128 eight accumulators over the first n - n % 8
// elements, combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder in order.  F maps an element to its term.
template <class F>
__device__ __forceinline__ double evo_np_sum(const double *x, int n, int stride, F term) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; i++) res = res + term(x[(size_t)i * stride]);
    return res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = term(x[(size_t)j * stride]);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = r[j] + term(x[(size_t)(i + j) * stride]);
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; i++) res = res + term(x[(size_t)i * stride]);
  return res + 0.0;  // (numpy adds the sum to its initial 0.0: a sum of -0.0 comes out as +0.0)
}

__global__ __launch_bounds__(64) void evo_aggregate_kernel(const EvoAggregateArgs a) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= a.G) return;
  const int S = a.S, D = a.D;
  const double nan = __longlong_as_double(0x7ff8000000000000ll), dS = (double)S;
  const int32_t *ns = a.n_step + (size_t)g * S;
  int32_t t = 0;
  bool valid = true;
  for (int s = 0; s < S; s++) {
    const int32_t v = ns[s];
    valid = valid && v >= 0;
    t = (int32_t)((uint32_t)t + (uint32_t)v);
  }
  const double *ob = a.objective + (size_t)g * S;
  double acc = 0.0;
  for (int s = 0; s < S; s++) acc = acc + ob[s];
  const double *bh = a.behaviours + (size_t)g * S * D;
  double stds = 0.0;
  for (int j = 0; j < D; j++) {
    const double mean = evo_np_sum(bh + j, S, D, [](double v) { return v; }) / dS;
    const double var = evo_np_sum(bh + j, S, D, [mean](double v) { return (v - mean) * (v - mean); }) / dS;
    const double sd = __dsqrt_rn(var);
    stds = j == 0 ? sd : stds + sd;
    a.out_behaviours[(size_t)g * D + j] = valid ? mean : nan;
  }
  a.out_objective[g] = valid ? (a.weight * acc) / dS : nan;
  a.out_time[g] = (int32_t)(0u - (uint32_t)t);
  a.out_variance[g] = -stds / (double)D;
  a.out_valid[g] = valid ? 1 : 0;
}

#endif  // PCGRL_ARCHIVE_KERNEL

}  // namespace pcgrl
