// smb/pcgrl_smb_vector.h -- the float32 hand-out of Super Mario Bros environments (include/pcgrl_amd_smb_vector.h): the
// observation RLlib's Box declares, float32 [oh][ow][2K + 8] with the env's 2K control values as constant planes in front of the
// one-hot channels (control_wrappers.py:189-214), written once and in its final form.  DESIGN.md section 23.
//
// One 64-lane wave per env -- at small batches several, each with a slice of the env's run (below).  The image is a function
// of the env's map (16-byte loads into LDS, as smb_env_load_map), its position and the 2K floats of the handle's control
// observation, so nothing of the uint8 observation is read: the kernel never touches it.
//   run       an env's image is one flat run of F = oh * ow * C floats (C = 2K + 8, always even, so F is even and an env's
//             run starts on 8 bytes whenever `out` does).  A lane produces four consecutive floats and stores them as 16 bytes;
//             the lanes of a wave cover 1 KiB of consecutive addresses per pass.
//   cases     C is a multiple of 4 for even K; for odd K it is not, and F is a multiple of 4 only when oh * ow is even.  So an
//             env's run starts on 16 bytes (K even; K odd with oh * ow even; every even env otherwise, given a 16-byte `out`)
//             or on 8 only (K odd with oh * ow odd: every odd env; or an `out` on 8).  A run on 8 only is stored as a 2-float head
//             (8 bytes), 16-byte quads from the next 16-byte boundary on, and a 2-float tail (8 bytes) where two are left.
//   values    float f of the run is cell f / C, channel f % C.  A lane divides once, before the loop; per pass it advances cell,
//             channel, window row and column by the constant stride (256 floats per slice) with carries.  A quad spans at
//             most two cells (C >= 8).
//   slices    one wave stores 1 KiB per pass, so with one wave per env a batch of 20 (the reference's envs per worker) would keep
//             20 of the chip's 1 024 SIMDs busy for 232 passes each.  The grid is (n, S): wave s of an env takes quads
//             64 s + lane, then every 64 S-th.  The launcher picks S = 2 048 / n, so that about 2 048 waves run: S = 1 above
//             1 024 envs, never more than the run has passes, at most 256.  Every wave loads the map for itself (2 KiB).
//   stores    plain 16-byte (8-byte) vector stores; `out` may be device memory or host-mapped pinned memory.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcgrl_smb_env.h"

namespace pcgrl {

struct SmbVectorArgs {
  int32_t h, w, oh, ow, n, map_stride, n_ctrl;
  const uint8_t *maps;       // [n][map_stride]
  const SmbEnvState *st;     // [n]
  const float *ctrl_obs;     // [n][2 * n_ctrl], null without controls
  float *out;                // [n][oh][ow][2 * n_ctrl + 8]
};

hipError_t launch_smb_vector_obs(const SmbVectorArgs &a, hipStream_t s);

#ifdef PCGRL_SMB_VECTOR_KERNEL  // (smb/pcgrl_k_smb_vector.hip has it; nothing of the other smb kernels is needed)

struct SmbVectorLds {
  uint8_t map[SMB_MAX_H * SMB_MAX_W];
  float ctrl[2 * SMB_STATS];
};

__global__ __launch_bounds__(64) void smb_vector_obs_kernel(const SmbVectorArgs a) {
  __shared__ __attribute__((aligned(16))) SmbVectorLds L;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= a.n) return;
  {
    const uint4 *src = (const uint4 *)(a.maps + (size_t)env * a.map_stride);
    for (int i = lane; i < a.map_stride / 16; i += 64) ((uint4 *)L.map)[i] = src[i];
  }
  const int K2 = 2 * a.n_ctrl;
  if (lane < K2) L.ctrl[lane] = a.ctrl_obs[(size_t)env * K2 + lane];
  const int H = a.h, W = a.w;
  const uint32_t OW = (uint32_t)a.ow, C = (uint32_t)(K2 + 8), F = (uint32_t)(a.oh * a.ow) * C;
  const int r0 = a.st[env].pos[0] - a.oh / 2, c0 = a.st[env].pos[1] - a.ow / 2;
  float *base = a.out + (size_t)env * F;
  __syncthreads();
  // the one-hot channel of window cell (r, c): 0 outside the map, 1 + tile inside
  auto code = [&](uint32_t r, uint32_t c) -> uint32_t {
    const int mr = r0 + (int)r, mc = c0 + (int)c;
    return (mr >= 0 && mr < H && mc >= 0 && mc < W) ? 1u + L.map[mr * W + mc] : 0u;
  };
  auto value = [&](uint32_t ch, uint32_t cd) -> float {
    return ch < (uint32_t)K2 ? L.ctrl[ch] : (ch - (uint32_t)K2 == cd ? 1.0f : 0.0f);
  };
  // two floats at f (even, f + 2 <= F): the head and the tail of a run that starts on 8 bytes only
  auto pair = [&](uint32_t f) {
    const uint32_t cell = f / C, ch = f - cell * C;  // (C is even: both floats are of one cell)
    const uint32_t r = cell / OW, cd = code(r, cell - r * OW);
    *(float2 *)(base + f) = make_float2(value(ch, cd), value(ch + 1, cd));
  };
  const uint32_t head = ((uintptr_t)base & 8u) ? 2u : 0u;
  const uint32_t nq = (F - head) >> 2, rest = head + (nq << 2);
  const uint32_t S = gridDim.y, slice = blockIdx.y;
  if (slice == 0) {
    if (head && lane == 0) pair(0);
    if (rest < F && lane == 1) pair(rest);
  }
  // the quads: lane l of slice s takes quads 64 s + l, then every 64 S-th; per pass every index advances by 256 S floats
  uint32_t q = slice * 64u + (uint32_t)lane;
  if (q >= nq) return;
  const uint32_t qstep = 64u * S, fstep = 256u * S;
  uint32_t f = head + (q << 2);
  uint32_t cell = f / C, ch = f - cell * C;
  uint32_t r = cell / OW, c = cell - r * OW;
  const uint32_t dcell = fstep / C, dch = fstep - dcell * C, drow = dcell / OW, dcol = dcell - drow * OW;
  for (; q < nq; q += qstep) {
    const uint32_t cd0 = code(r, c);
    const uint32_t c1 = c + 1 == OW ? 0u : c + 1, r1 = c + 1 == OW ? r + 1 : r;
    // (cd1 is selected only by floats of the next cell; a quad lies inside the run, so it has none past the last cell)
    const uint32_t cd1 = code(r1, c1);
    float v[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      const uint32_t cj = ch + j;
      v[j] = cj < C ? value(cj, cd0) : value(cj - C, cd1);
    }
    *(float4 *)(base + f) = make_float4(v[0], v[1], v[2], v[3]);
    f += fstep;
    ch += dch;
    uint32_t carry = 0;
    if (ch >= C) {
      ch -= C;
      carry = 1;
    }
    c += dcol + carry;  // dcol <= OW - 1: one subtraction is enough
    r += drow;
    if (c >= OW) {
      c -= OW;
      r++;
    }
  }
}

#endif  // PCGRL_SMB_VECTOR_KERNEL

}  // namespace pcgrl
