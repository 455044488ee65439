// nca/pcgrl_nca.h -- the NCA level generator on the device (include/pcgrl_amd_nca.h has the rules, DESIGN.md section 38 the
// reasoning; control_pcgrl_amd/nca.py is the same in numpy).
//
// One workgroup rolls out one (genome, seed) pair from the init map to the final map: no kernel boundary between steps.
//   LDS   the genome, re-laid for the reads below; two copies of the byte map (read one, write the other, swap); three flag
//         words that rotate (step n ORs into flag[n % 3], everybody reads it after the step's one barrier, thread 0 clears
//         flag[(n + 2) % 3] for the step after next: the stop test costs one barrier per step)
//   lane  CPL cells per pass, a pass covering blockDim * CPL cells; the library runs CPL = 1 (a 16 x 16 map is one pass of 256
//         lanes, a 64 x 64 map sixteen); CPL = 2 is a development build, measured 1-9 % slower
//   layer 1  the one-hot input turns the 3 x 3 convolution into at most nine adds per output channel, but the stated order is
//         by (tile, ky, kx): the lane sorts its taps by that key once per cell (36 compares, the order packed 7 bits a key
//         into a uint64), then reads w1t[key][o] -- [T * 9] rows of 32 floats padded to 36, so that 16 lanes with 16 different
//         keys hit 16 different 16-byte bank slots -- four output channels per ds_read_b128
//   layers 2, 3  h1[32] stays in registers; for o = 0..31 the row w2[o][0..31] comes as eight ds_read_b128 at an address all
//         lanes share (a broadcast: 4 LDS cycles each, for 64 v_mul + v_add per cell); h2[o] is folded into the T layer-3
//         accumulators at once -- acc3[i] += w3[i][o] * h2[o] for ascending o is the stated order
//   pick  the first index of the largest logit, j.  s32 is monotone, so s32(logit[j]) is the largest sigmoid and only an i < j
//         with the same float32 sigmoid can win.  A channel with lmax - l > 1, l < 12 and lmax > -87 cannot tie: there
//         s(l + 1) / s(l) >= 1 + 3.8e-6, thirty float32 spacings, and s(lmax) is a normal float32; every other i < j is evaluated.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

namespace pcgrl {

constexpr int NCA_HID = 32;
constexpr int NCA_MIN_T = 2;
constexpr int NCA_MAX_T = 8;
constexpr int NCA_MAX_SIDE = 64;
constexpr int NCA_MAX_STEPS = 1024;
constexpr int NCA_MAX_THREADS = 256;
constexpr int NCA_W1_STRIDE = 36;  // floats per (tile, tap) row of w1t
constexpr uint32_t NCA_MAGIC = 0x4E514350u;  // "PCQN"

struct NcaArgs {
  int32_t H, W, S, n_steps, init_per_genome;
  const float *weights;  // [G][P]
  const uint8_t *init;   // [S][H][W] or [G][S][H][W]
  uint8_t *levels;       // [G][S][H][W]
  int32_t *n_step;       // [G][S]
  uint8_t *frames;       // [G][S][n_steps][H][W] or null
  uint32_t *error;       // [1]
};

constexpr int nca_tp(int T) { return (T + 3) / 4 * 4; }
constexpr int nca_params(int T) { return 9 * T * NCA_HID + NCA_HID + NCA_HID * NCA_HID + NCA_HID + T * NCA_HID + T; }
// floats of LDS in front of the two maps
constexpr int nca_lds_floats(int T) { return T * 9 * NCA_W1_STRIDE + 32 + 1024 + 32 + 32 * nca_tp(T) + 8 + 4; }
inline size_t nca_lds_bytes(int T, int cells) { return (size_t)nca_lds_floats(T) * 4 + 2 * (size_t)((cells + 15) / 16 * 16); }

hipError_t launch_nca(int T, int64_t pairs, const NcaArgs &a, hipStream_t s);

#ifdef PCGRL_NCA_KERNEL
#pragma clang fp contract(off)  // every multiply and every add is rounded on its own

__device__ __forceinline__ float nca_relu(float a) { return a < 0.0f ? 0.0f : a; }

// the float32 sigmoid of the header, in double with + - * / only
__device__ __forceinline__ float nca_s32(float xf) {
  const double x = (double)xf;
  const double z = -fmin(fabs(x), 104.0);
  const double k = rint(z * 1.4426950408889634);
  const double r = (z - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
  double p = 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 1.0 / 2.0;
  p = p * r + 1.0;
  p = p * r + 1.0;
  const double t = ldexp(p, (int)k);
  return (float)((x >= 0.0 ? 1.0 : t) / (1.0 + t));
}

// layers 2 and 3 of CPL cells whose h1 is in registers: logits into acc3 (the stated order: ascending input channel from the
// bias).  w2 [32][32] as in the genome, w3t [32][TP] (w3[i][c] at c * TP + i, zero-padded), all in LDS; the 3-D generator
// (nca3d/pcgrl_nca3d.h) calls this too.
template <int T, int CPL>
__device__ __forceinline__ void nca_layers23(const float (&h1)[CPL][NCA_HID], const float *w2, const float *b2,
                                             const float *w3t, const float *b3, float (&acc3)[CPL][T]) {
  constexpr int TP = nca_tp(T);
#pragma unroll
  for (int k = 0; k < CPL; k++) {
#pragma unroll
    for (int i = 0; i < T; i++) acc3[k][i] = b3[i];
  }
#pragma unroll 1
  for (int o = 0; o < NCA_HID; o++) {
    float wr[NCA_HID], w3r[TP];
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const float4 v = ((const float4 *)(w2 + o * 32))[q];
      wr[q * 4 + 0] = v.x, wr[q * 4 + 1] = v.y, wr[q * 4 + 2] = v.z, wr[q * 4 + 3] = v.w;
    }
#pragma unroll
    for (int q = 0; q < TP / 4; q++) {
      const float4 v = ((const float4 *)(w3t + o * TP))[q];
      w3r[q * 4 + 0] = v.x, w3r[q * 4 + 1] = v.y, w3r[q * 4 + 2] = v.z, w3r[q * 4 + 3] = v.w;
    }
    const float bias = b2[o];
#pragma unroll
    for (int k = 0; k < CPL; k++) {
      float acc = bias;
#pragma unroll
      for (int c = 0; c < NCA_HID; c++) acc = acc + wr[c] * h1[k][c];
      const float h2 = nca_relu(acc);
#pragma unroll
      for (int i = 0; i < T; i++) acc3[k][i] = acc3[k][i] + w3r[i] * h2;
    }
  }
}

// the pick: the first index at which s32(logit) is largest (the shortcut is in the head of this file); `finite` says whether
// every logit is finite
template <int T>
__device__ __forceinline__ int nca_pick(const float (&logit)[T], bool &finite) {
  float lmax = logit[0];
  int j = 0;
  finite = fabsf(logit[0]) <= FLT_MAX;
#pragma unroll
  for (int i = 1; i < T; i++) {
    finite = finite && fabsf(logit[i]) <= FLT_MAX;
    if (logit[i] > lmax) lmax = logit[i], j = i;
  }
  int win = j;
  if (j > 0 && finite) {
    const float smax = nca_s32(lmax);
#pragma unroll
    for (int i = T - 2; i >= 0; i--) {
      const float l = logit[i];
      const bool cannot_tie = lmax - l > 1.0f && l < 12.0f && lmax > -87.0f;
      if (i < j && !cannot_tie && nca_s32(l) == smax) win = i;
    }
  }
  return win;
}

template <int T, int CPL>
__global__ void __launch_bounds__(NCA_MAX_THREADS) nca_kernel(NcaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nca_smem[];
  constexpr int TP = nca_tp(T);
  constexpr int P = nca_params(T);
  constexpr int O_B1 = 9 * T * NCA_HID, O_W2 = O_B1 + 32, O_B2 = O_W2 + 1024, O_W3 = O_B2 + 32, O_B3 = O_W3 + 32 * T;
  float *w1t = (float *)nca_smem;               // [T * 9][36]: w1[o][c][tap] at (c * 9 + tap) * 36 + o
  float *b1 = w1t + T * 9 * NCA_W1_STRIDE;      // [32]
  float *w2 = b1 + 32;                          // [32][32] as in the genome
  float *b2 = w2 + 1024;                        // [32]
  float *w3t = b2 + 32;                         // [32][TP]: w3[i][c] at c * TP + i
  float *b3 = w3t + 32 * TP;                    // [8]
  uint32_t *flag = (uint32_t *)(b3 + 8);        // [4], three in use
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int H = a.H, W = a.W, cells = H * W;
  uint8_t *cur = (uint8_t *)(flag + 4);
  uint8_t *nxt = cur + (cells + 15) / 16 * 16;
  const size_t pair = blockIdx.x;
  const size_t g = pair / (size_t)a.S, s = pair - g * (size_t)a.S;

  const float *wg = a.weights + g * (size_t)P;
  for (int i = tid; i < P; i += nthr) {
    const float v = wg[i];
    if (i < O_B1) {
      const int o = i / (T * 9), r = i - o * (T * 9);
      w1t[r * NCA_W1_STRIDE + o] = v;
    } else if (i < O_W2) {
      b1[i - O_B1] = v;
    } else if (i < O_B2) {
      w2[i - O_W2] = v;
    } else if (i < O_W3) {
      b2[i - O_B2] = v;
    } else if (i < O_B3) {
      const int j = i - O_W3, ti = j >> 5, c = j & 31;
      w3t[c * TP + ti] = v;
    } else {
      b3[i - O_B3] = v;
    }
  }
  if (TP > T)
    for (int i = tid; i < 32 * (TP - T); i += nthr) w3t[(i / (TP - T)) * TP + T + i % (TP - T)] = 0.0f;
  if (tid < 3) flag[tid] = 0;
  const uint8_t *im = a.init + (a.init_per_genome ? pair : s) * (size_t)cells;
  int bad = 0;
  for (int i = tid; i < cells; i += nthr) {
    const uint8_t t = im[i];
    cur[i] = t;
    bad |= t >= T;
  }
  uint8_t *lv = a.levels + pair * (size_t)cells;
  uint8_t *fr = a.frames ? a.frames + pair * (size_t)a.n_steps * (size_t)cells : nullptr;
  uint32_t err = __syncthreads_or(bad) ? 1u : 0u;  // (the barrier after the staging as well)

  int step = 0;
  if (!err) {
    for (;; ++step) {
      uint32_t mine = 0;
      for (int base = 0; base < cells; base += nthr * CPL) {
        float h1[CPL][NCA_HID];
#pragma unroll
        for (int k = 0; k < CPL; k++) {
          const int cell = base + k * nthr + tid;
          const int cc = cell < cells ? cell : 0;
          const int y = cc / W, x = cc - y * W;
          // the taps in the stated order: sorted by tile * 9 + tap, those outside the map last
          int key[9], rank[9], nv = 0;
#pragma unroll
          for (int tap = 0; tap < 9; tap++) {
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            const bool inside = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            const int t = cur[inside ? yy * W + xx : cc];
            key[tap] = inside ? t * 9 + tap : 127;
            nv += inside;
            rank[tap] = 0;
          }
#pragma unroll
          for (int t = 1; t < 9; t++) {
#pragma unroll
            for (int u = 0; u < t; u++) {
              const int lt = key[u] < key[t];
              rank[t] += lt;
              rank[u] += 1 - lt;
            }
          }
          unsigned long long pk = 0;
#pragma unroll
          for (int tap = 0; tap < 9; tap++) pk |= (unsigned long long)key[tap] << (7 * rank[tap]);
          int kj[9];
#pragma unroll
          for (int j = 0; j < 9; j++) kj[j] = j < nv ? (int)((pk >> (7 * j)) & 127u) * NCA_W1_STRIDE : 0;  // the row's float index
#pragma unroll
          for (int oq = 0; oq < 8; oq++) {
            float4 acc = ((const float4 *)b1)[oq];
#pragma unroll
            for (int j = 0; j < 9; j++) {
              const float4 w = *(const float4 *)(w1t + kj[j] + oq * 4);
              const bool on = j < nv;
              acc.x = on ? acc.x + w.x : acc.x;
              acc.y = on ? acc.y + w.y : acc.y;
              acc.z = on ? acc.z + w.z : acc.z;
              acc.w = on ? acc.w + w.w : acc.w;
            }
            h1[k][oq * 4 + 0] = nca_relu(acc.x);
            h1[k][oq * 4 + 1] = nca_relu(acc.y);
            h1[k][oq * 4 + 2] = nca_relu(acc.z);
            h1[k][oq * 4 + 3] = nca_relu(acc.w);
            // the next quad's reads wait for this quad's sums: nine reads in flight, not all 72 of them
            asm volatile("" : "+v"(kj[0]), "+v"(kj[1]), "+v"(kj[2]), "+v"(kj[3]), "+v"(kj[4]), "+v"(kj[5]), "+v"(kj[6]),
                         "+v"(kj[7]), "+v"(kj[8]), "+v"(h1[k][oq * 4 + 0]), "+v"(h1[k][oq * 4 + 1]), "+v"(h1[k][oq * 4 + 2]),
                         "+v"(h1[k][oq * 4 + 3]));
          }
        }
        float acc3[CPL][T];
        nca_layers23<T, CPL>(h1, w2, b2, w3t, b3, acc3);
#pragma unroll
        for (int k = 0; k < CPL; k++) {
          const int cell = base + k * nthr + tid;
          bool finite;
          const int win = nca_pick<T>(acc3[k], finite);
          if (cell < cells) {
            nxt[cell] = (uint8_t)win;
            mine |= (win != cur[cell] ? 1u : 0u) | (finite ? 0u : 2u);
            if (fr) fr[(size_t)step * (size_t)cells + cell] = (uint8_t)win;
          }
        }
      }
      if (mine) atomicOr(&flag[step % 3], mine);
      __syncthreads();
      const uint32_t f = flag[step % 3];
      if (tid == 0) flag[(step + 2) % 3] = 0;
      uint8_t *const swap = cur;
      cur = nxt, nxt = swap;
      if (f & 2u) {
        err = 2u;
        break;
      }
      if (!(f & 1u) || step >= a.n_steps - 1) break;
    }
  }

  if (err) {  // refused: the init map everywhere, -1
    for (int i = tid; i < cells; i += nthr) {
      const uint8_t t = im[i];
      lv[i] = t;
      if (fr)
        for (int r = 0; r < a.n_steps; r++) fr[(size_t)r * (size_t)cells + i] = t;
    }
    if (tid == 0) {
      a.n_step[pair] = -1;
      atomicOr(a.error, err);
    }
    return;
  }
  for (int i = tid; i < cells; i += nthr) {
    const uint8_t t = cur[i];
    lv[i] = t;
    if (fr)
      for (int r = step + 1; r < a.n_steps; r++) fr[(size_t)r * (size_t)cells + i] = t;
  }
  if (tid == 0) a.n_step[pair] = step;
}

#endif  // PCGRL_NCA_KERNEL

}  // namespace pcgrl
