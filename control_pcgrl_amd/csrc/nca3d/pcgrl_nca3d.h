// nca3d/pcgrl_nca3d.h -- the 3-D NCA level generator on the device, plain and holey (include/pcgrl_amd_nca3d.h has the rules,
// DESIGN.md section 44 the reasoning; control_pcgrl_amd/nca3d.py is the same in numpy).  Layers 2 and 3, nca_s32 and the pick
// are the 2-D generator's (nca/pcgrl_nca.h: nca_layers23, nca_pick); layer 1, the image and the staging are this file's.
//
// One workgroup rolls out one (genome, seed) pair from the init map to the final map: no kernel boundary between steps.
//   LDS   the genome, re-laid for the reads below; two copies of the byte IMAGE -- the map inside a one-cell ring,
//         [D0 + 2][D1 + 2][D2 + 2] -- read one, write the other, swap; the three rotating flag words of the 2-D kernel (the stop
//         test costs one barrier per step).  The ring is written once, into both copies: NCA3D_NO_TAP (255) in plain mode, the
//         border tile with the four hole cells in holey mode.  Both modes then run the same loop: a tap whose byte is below T
//         adds its weight, any other byte adds nothing, and only interior cells are computed, compared and written.
//   lane  one cell per pass.  Block size: passes = ceil(cells / 256), lanes = ceil(cells / passes) rounded up to 64 -- the
//         fewest passes, and then the fewest idle lanes in them: 3^3 = 27 cells run on 64 lanes, 5^3 = 125 on 128, 7^3 = 343 in
//         two passes of 192 (not a pass and a third of 256), 15^3 in 14 passes of 256, 16^3 in 16.
//   layer 1  the one-hot input turns the 3 x 3 x 3 convolution into at most 27 adds per output channel, in TAP order (the
//         rule): the 32 sums stay in registers and the taps are walked (k0, k1, k2) ascending, in nine rolled rounds of
//         three; a tap reads its byte (a round ahead), then the
//         row w1t[tile * 27 + tap] -- [T * 27] rows of 32 floats padded to 36 -- as eight ds_read_b128.  The lanes of a wave are
//         at the same tap, so they differ in the tile alone: rows 27 * 36 floats apart, 12 banks modulo 64, which puts the up
//         to eight different rows of one read in eight different 16-byte bank slots (0, 12, 24, 36, 48, 60, 8, 20).
//   layers 2, 3 and the pick  nca_layers23<T, 1> and nca_pick<T>
#pragma once
#include "../nca/pcgrl_nca.h"

namespace pcgrl {

constexpr int NCA3D_TAPS = 27;
constexpr int NCA3D_MIN_AXIS = 3;
constexpr int NCA3D_MAX_AXIS = 16;
constexpr int NCA3D_NO_TAP = 255;
constexpr uint32_t NCA3D_ERR_TILE = 1u, NCA3D_ERR_NONFINITE = 2u, NCA3D_ERR_HOLE = 4u;
constexpr uint32_t NCA3D_MAGIC = 0x33514350u;  // "PCQ3"

struct Nca3dArgs {
  int32_t D0, D1, D2, S, n_steps, init_per_genome, holey, holes_per_seed, border_tile, empty_tile;
  const float *weights;  // [G][P]
  const uint8_t *init;   // [S][D0][D1][D2] or [G][S][D0][D1][D2]
  const int32_t *holes;  // [2][3] or [S][2][3], foot cells (z, y, x) in image coordinates; null in plain mode
  uint8_t *levels;       // [G][S][D0][D1][D2]
  int32_t *n_step;       // [G][S]
  uint8_t *frames;       // [G][S][n_steps][D0][D1][D2] or null
  uint32_t *error;       // [1]
};

constexpr int nca3d_params(int T) { return NCA3D_TAPS * T * NCA_HID + NCA_HID + NCA_HID * NCA_HID + NCA_HID + T * NCA_HID + T; }
// floats of LDS in front of the two images
constexpr int nca3d_lds_floats(int T) { return T * NCA3D_TAPS * NCA_W1_STRIDE + 32 + 1024 + 32 + 32 * nca_tp(T) + 8 + 4; }
inline int nca3d_image_bytes(int d0, int d1, int d2) { return ((d0 + 2) * (d1 + 2) * (d2 + 2) + 15) / 16 * 16; }
inline size_t nca3d_lds_bytes(int T, int d0, int d1, int d2) {
  return (size_t)nca3d_lds_floats(T) * 4 + 2 * (size_t)nca3d_image_bytes(d0, d1, d2);
}
// the block size rule of the head of this file
inline int nca3d_threads(int cells) {
  const int passes = (cells + NCA_MAX_THREADS - 1) / NCA_MAX_THREADS;
  return ((cells + passes - 1) / passes + 63) / 64 * 64;
}

hipError_t launch_nca3d(int T, int64_t pairs, const Nca3dArgs &a, hipStream_t s);

#ifdef PCGRL_NCA3D_KERNEL
#pragma clang fp contract(off)  // every multiply and every add is rounded on its own

// mc3d_holey's hole_ok: the foot (z, y, x), in image coordinates, is on one of the four side faces, off the edges, and its head
// at z + 1 is below the top ring
__device__ __forceinline__ bool nca3d_hole_ok(int z, int y, int x, int D0, int D1, int D2) {
  return z >= 1 && z <= D0 - 1 &&
         (((x == 0 || x == D2 + 1) && y >= 1 && y <= D1) || ((y == 0 || y == D1 + 1) && x >= 1 && x <= D2));
}

template <int T>
__global__ void __launch_bounds__(NCA_MAX_THREADS) nca3d_kernel(Nca3dArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nca3d_smem[];
  constexpr int TP = nca_tp(T);
  constexpr int P = nca3d_params(T);
  constexpr int ROWS = T * NCA3D_TAPS;
  constexpr int O_B1 = ROWS * NCA_HID, O_W2 = O_B1 + 32, O_B2 = O_W2 + 1024, O_W3 = O_B2 + 32, O_B3 = O_W3 + 32 * T;
  float *w1t = (float *)nca3d_smem;             // [T * 27][36]: w1[o][c][tap] at (c * 27 + tap) * 36 + o
  float *b1 = w1t + ROWS * NCA_W1_STRIDE;       // [32]
  float *w2 = b1 + 32;                          // [32][32] as in the genome
  float *b2 = w2 + 1024;                        // [32]
  float *w3t = b2 + 32;                         // [32][TP]: w3[i][c] at c * TP + i
  float *b3 = w3t + 32 * TP;                    // [8]
  uint32_t *flag = (uint32_t *)(b3 + 8);        // [4], three in use
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int D0 = a.D0, D1 = a.D1, D2 = a.D2, plane = D1 * D2, cells = D0 * plane;
  const int R1 = D1 + 2, R2 = D2 + 2, ring_cells = (D0 + 2) * R1 * R2;
  uint8_t *cur = (uint8_t *)(flag + 4);
  uint8_t *nxt = cur + (ring_cells + 15) / 16 * 16;
  const size_t pair = blockIdx.x;
  const size_t g = pair / (size_t)a.S, s = pair - g * (size_t)a.S;

  const float *wg = a.weights + g * (size_t)P;
  for (int i = tid; i < P; i += nthr) {
    const float v = wg[i];
    if (i < O_B1) {
      const int o = i / ROWS, r = i - o * ROWS;
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

  // the holes of this seed, checked before anything is dug
  int hole[2][3] = {{0, 0, 0}, {0, 0, 0}};
  bool holes_ok = true;
  if (a.holey) {
    const int32_t *hp = a.holes + (a.holes_per_seed ? s * 6 : 0);
#pragma unroll
    for (int k = 0; k < 2; k++) {
      hole[k][0] = hp[k * 3 + 0], hole[k][1] = hp[k * 3 + 1], hole[k][2] = hp[k * 3 + 2];
      holes_ok = holes_ok && nca3d_hole_ok(hole[k][0], hole[k][1], hole[k][2], D0, D1, D2);
    }
  }
  // both images: the ring everywhere, then the interior of the first from the init map
  const uint8_t ring = a.holey ? (uint8_t)a.border_tile : (uint8_t)NCA3D_NO_TAP;
  for (int i = tid; i < ring_cells; i += nthr) cur[i] = ring, nxt[i] = ring;
  __syncthreads();
  if (a.holey && holes_ok && tid < 4) {
    const int k = tid >> 1, head = tid & 1;
    const int at = ((hole[k][0] + head) * R1 + hole[k][1]) * R2 + hole[k][2];  // inside the image: nca3d_hole_ok
    cur[at] = (uint8_t)a.empty_tile, nxt[at] = (uint8_t)a.empty_tile;
  }
  const uint8_t *im = a.init + (a.init_per_genome ? pair : s) * (size_t)cells;
  int bad = 0;
  for (int i = tid; i < cells; i += nthr) {
    const int z = i / plane, r = i - z * plane, y = r / D2, x = r - y * D2;
    const uint8_t t = im[i];
    cur[((z + 1) * R1 + (y + 1)) * R2 + (x + 1)] = t;
    bad |= t >= T;
  }
  uint8_t *lv = a.levels + pair * (size_t)cells;
  uint8_t *fr = a.frames ? a.frames + pair * (size_t)a.n_steps * (size_t)cells : nullptr;
  uint32_t err = (__syncthreads_or(bad) ? NCA3D_ERR_TILE : 0u) | (holes_ok ? 0u : NCA3D_ERR_HOLE);  // (the staging's barrier)

  int step = 0;
  if (!err) {
    for (;; ++step) {
      uint32_t mine = 0;
      for (int base = 0; base < cells; base += nthr) {
        const int cell = base + tid;
        const int cc = cell < cells ? cell : 0;
        const int z = cc / plane, r = cc - z * plane, y = r / D2, x = r - y * D2;
        const int centre = ((z + 1) * R1 + (y + 1)) * R2 + (x + 1);
        float h1[1][NCA_HID];
#pragma unroll
        for (int o = 0; o < NCA_HID; o++) h1[0][o] = b1[o];
        // nine rounds of three taps (k2 = 0, 1, 2), rolled: the 24 row reads of a round are all that is in flight, and the
        // three bytes of the next round are read ahead of them
        int t3[3];
#pragma unroll
        for (int k2 = 0; k2 < 3; k2++) t3[k2] = cur[centre - (R1 + 1) * R2 + (k2 - 1)];
#pragma unroll 1
        for (int k01 = 0; k01 < 9; k01++) {
          const int nk = k01 < 8 ? k01 + 1 : 8;  // (the last round reads its own bytes again)
          const int nat = centre + ((nk / 3 - 1) * R1 + (nk % 3 - 1)) * R2;
          int n3[3];
#pragma unroll
          for (int k2 = 0; k2 < 3; k2++) n3[k2] = cur[nat + (k2 - 1)];
#pragma unroll
          for (int k2 = 0; k2 < 3; k2++) {
            const int t = t3[k2];
            const bool on = t < T;
            const float *row = w1t + (on ? (t * NCA3D_TAPS + k01 * 3 + k2) * NCA_W1_STRIDE : 0);
#pragma unroll
            for (int oq = 0; oq < 8; oq++) {
              const float4 w = *(const float4 *)(row + oq * 4);
              h1[0][oq * 4 + 0] = on ? h1[0][oq * 4 + 0] + w.x : h1[0][oq * 4 + 0];
              h1[0][oq * 4 + 1] = on ? h1[0][oq * 4 + 1] + w.y : h1[0][oq * 4 + 1];
              h1[0][oq * 4 + 2] = on ? h1[0][oq * 4 + 2] + w.z : h1[0][oq * 4 + 2];
              h1[0][oq * 4 + 3] = on ? h1[0][oq * 4 + 3] + w.w : h1[0][oq * 4 + 3];
            }
          }
#pragma unroll
          for (int k2 = 0; k2 < 3; k2++) t3[k2] = n3[k2];
        }
#pragma unroll
        for (int o = 0; o < NCA_HID; o++) h1[0][o] = nca_relu(h1[0][o]);
        float acc3[1][T];
        nca_layers23<T, 1>(h1, w2, b2, w3t, b3, acc3);
        bool finite;
        const int win = nca_pick<T>(acc3[0], finite);
        if (cell < cells) {
          nxt[centre] = (uint8_t)win;
          mine |= (win != cur[centre] ? 1u : 0u) | (finite ? 0u : 2u);
          if (fr) fr[(size_t)step * (size_t)cells + cell] = (uint8_t)win;
        }
      }
      if (mine) atomicOr(&flag[step % 3], mine);
      __syncthreads();
      const uint32_t f = flag[step % 3];
      if (tid == 0) flag[(step + 2) % 3] = 0;
      uint8_t *const swap = cur;
      cur = nxt, nxt = swap;
      if (f & 2u) {
        err = NCA3D_ERR_NONFINITE;
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
    const int z = i / plane, r = i - z * plane, y = r / D2, x = r - y * D2;
    const uint8_t t = cur[((z + 1) * R1 + (y + 1)) * R2 + (x + 1)];
    lv[i] = t;
    if (fr)
      for (int q = step + 1; q < a.n_steps; q++) fr[(size_t)q * (size_t)cells + i] = t;
  }
  if (tid == 0) a.n_step[pair] = step;
}

#endif  // PCGRL_NCA3D_KERNEL

}  // namespace pcgrl
