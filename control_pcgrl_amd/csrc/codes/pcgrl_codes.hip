// codes/pcgrl_codes.hip -- translation unit: the tile-code observation kernels (see codes/pcgrl_codes.h).
//
// codes_observe_kernel: one group of LPE lanes per env, one lane per map row, like observe_kernel (pcgrl_kernels2d.h).  Each
// lane loads its row's tile bit-planes and writes the row's codes into LDS; the group then streams the env's codes out in
// 16-byte chunks (store_obs16) covering whole cache lines, lane r taking chunks r, r + LPE, ...  The bytes before the first
// 16-byte boundary of the env's row and after the last one -- windows of any byte count, rows that start unaligned -- are
// plain byte stores.  Two forms:
//   PAD (one plane, LDS permitting: every BASELINE config)  like encode_obs_codes, a map row is kept ZERO-PADDED: PADL zero
//        bytes, the W codes (written as dwords from the bit-planes: spread4 / nibble_at), zeros up to the row stride RS, so a
//        window row is a contiguous slice of a padded row (or of the shared zero row above / below the map).  A chunk that
//        lies inside one window row is five aligned LDS dwords and four v_alignbyte; only chunks that straddle two window
//        rows (windows whose width is not a multiple of 16) go byte by byte.  LDS per env: H * RS bytes (1 KB at 16 x 16 with
//        the 32 x 32 window).
//   generic (the static plane, or windows too wide for the padded rows)  unpadded codes [H][W] and the bordered static mask
//        [H + 2][W + 2] in LDS, every output byte looked up with bounds tests.  LDS per env <= 8.3 KB.
// Binary 16 x 16 with the 32 x 32 window (the compile-time step kernels): the step launch without an observation leaves the
// pre-flooded component of the next edit cell invalid (pcgrl_kernels2d.h PREFLOOD -- the observe wave computes it after its
// stores).  The PAD kernel computes it the same way after ITS stores, so the next step keeps the flood off its critical path.
#include <algorithm>

#define PCGRL_KERNEL_TU
#include "../pcgrl_dispatch.h"
#include "pcgrl_codes.h"

namespace pcgrl {

__device__ inline size_t codes_env_lds(int H, int W, int P) {
  return ((size_t)H * W + (P > 1 ? (size_t)(H + 2) * (W + 2) : 0) + 15) & ~(size_t)15;
}

template <int PROB, int LPE, typename M, bool PAD>
// (8 waves per SIMD asked of the compiler for the padded form; the generic form with 64-bit row masks would spill under that
// bound and keeps 7)
__global__ __launch_bounds__(64, PAD ? 8 : 1) void codes_observe_kernel(Params p, CodesArgs a) {
  constexpr int NB = ProbTraits<PROB>::NB, EPW = 64 / LPE;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  Grp<LPE> g;
  g.init();
  const int env = blockIdx.x * EPW + (g.lane / LPE);
  const bool active = env < p.n_envs;
  const int e = active ? env : 0;
  const int H = p.cfg.dims[0], W = p.cfg.dims[1];
  const bool rowok = active && g.row < H;
  M b[NB];
  load_planes<NB, M>(p, e, g.row, rowok, b);
  const int pos0 = p.st[e].pos[0], pos1 = p.st[e].pos[1];
  const int OH = a.wide ? H : p.cfg.obs_window[0], OW = a.wide ? W : p.cfg.obs_window[1];
  const int top = a.wide ? 0 : pos0 - OH / 2, left = a.wide ? 0 : pos1 - OW / 2;
  const int T = a.T;
  uint8_t *dst = a.out + (size_t)env * (size_t)T;
  const int head = min(T, (int)((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u));
  const int nch = (T - head) >> 4, tail = head + 16 * nch;
  auto put = [&](int t0, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    const uint4 v = make_uint4(w0, w1, w2, w3);
    if (a.nt)
      store_obs16_nt(dst + (size_t)t0, v);
    else
      store_obs16(dst + (size_t)t0, v);
  };
  if constexpr (PAD) {
    const int RS = a.rs, PADL = a.pad_l;
    uint8_t *rows = lds + (size_t)(g.lane / LPE) * H * RS;  // this env's padded code rows
    uint8_t *zero_row = lds + (size_t)EPW * H * RS;         // what a window row above / below the map reads
    const M inmap = W >= (int)(8 * sizeof(M)) ? ~M(0) : ((M(1) << W) - M(1));
    if (g.row < H) {
      uint8_t *row = rows + g.row * RS;
      for (int o = 0; o < RS; o += 16) {
        uint32_t w[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
          const int x0 = o + 4 * t - PADL;  // map column of the dword's first byte (PADL is a multiple of 4)
          uint32_t v = 0;
          if (x0 >= 0 && x0 < W) {
            v = a.wide ? 0u : spread4(nibble_at<M>(inmap, x0));  // (cropped: 1 + tile)
#pragma unroll
            for (int k = 0; k < NB; k++) v += spread4(nibble_at<M>(b[k] & inmap, x0)) << k;
          }
          w[t] = v;
        }
        *(uint4 *)(row + o) = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
    for (int o = g.lane * 16; o < RS; o += 64 * 16) *(uint4 *)(zero_row + o) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    if (active) {
      const int off0 = PADL + left;  // padded index of window column 0 (>= 0)
      auto rowp = [&](int i) -> const uint8_t * {
        const int m = top + i;
        return (unsigned)m < (unsigned)H ? rows + m * RS : zero_row;
      };
      auto at = [&](int t) -> uint32_t {
        const int i = t / OW;
        return rowp(i)[off0 + t - i * OW];
      };
      for (int t = g.row; t < head; t += LPE) dst[t] = (uint8_t)at(t);
      for (int t = tail + g.row; t < T; t += LPE) dst[t] = (uint8_t)at(t);
      for (int k = g.row; k < nch; k += LPE) {
        const int t0 = head + 16 * k;
        int i = t0 / OW, j = t0 - i * OW;
        const uint8_t *rp = rowp(i);
        if (j + 16 <= OW) {  // one window row: 16 contiguous bytes of a padded row
          const uintptr_t src = (uintptr_t)(rp + off0 + j);
          const uint32_t *d = (const uint32_t *)(src & ~(uintptr_t)3);
          const uint32_t sh = (uint32_t)(src & 3u);
          const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
          put(t0, __builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
              __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh));
        } else {  // the chunk straddles window rows
          uint32_t w[4] = {0u, 0u, 0u, 0u};
          for (int n = 0; n < 16; n++) {
            w[n >> 2] |= (uint32_t)rp[off0 + j] << (8 * (n & 3));
            if (++j == OW) {
              j = 0;
              rp = rowp(++i);
            }
          }
          put(t0, w[0], w[1], w[2], w[3]);
        }
      }
    }
    if constexpr (PROB == PCGRL_PROB_BINARY && LPE == 16 && sizeof(M) == 4) {
      if (a.pre) {  // (see the header: what the step kernel's observe wave leaves for the next step)
        const M colmask = rowok ? inmap : M(0);
        const M xbit = (rowok && g.row == pos0) ? (M(1) << pos1) : M(0);
        const M comp = flood(g, xbit, (~b[0] & colmask) | xbit);
        if (rowok) ((M *)p.planes)[((size_t)e * ROW_WORDS + PRE_PLANE) * H + g.row] = comp | (M)PRE_VALID;
      }
    }
  } else {
    const int P = a.P, BW = W + 2, RB = OW * P;
    uint8_t *cm = lds + (size_t)(g.lane / LPE) * codes_env_lds(H, W, P);  // this env's codes [H][W]
    uint8_t *sm = cm + (size_t)H * W;                                       // ... and bordered static mask [H + 2][W + 2]
    if (g.row < H) {
      const int base = a.wide ? 0 : 1;
      uint8_t *row = cm + g.row * W;
      for (int x = 0; x < W; x++) row[x] = (uint8_t)(base + tile_at<NB, M>(b, x));
    }
    if (P > 1) {
      ExtRow<NB, M> X;
      X.load(p, e, g.row, rowok);
      if (g.row < H) {  // bordered row r + 1: the ring cells and the protection of map row r
        uint8_t *row = sm + (g.row + 1) * BW;
        row[0] = 1;
        row[W + 1] = 1;
        for (int x = 0; x < W; x++) row[x + 1] = (uint8_t)((X.prot >> x) & M(1));
      }
      if (g.row < 2) {  // bordered rows 0 and H + 1: all ring
        uint8_t *row = sm + (g.row == 0 ? 0 : (H + 1) * BW);
        for (int x = 0; x < BW; x++) row[x] = 1;
      }
    }
    __syncthreads();
    if (!active) return;
    // byte t of the env's codes: window row i = t / RB, column j, plane c  ->  map cell (top + i, left + j)
    auto cell = [&](int r, int q, int c) -> uint32_t {
      if (c == 0) return ((unsigned)r < (unsigned)H && (unsigned)q < (unsigned)W) ? cm[r * W + q] : 0u;
      return ((unsigned)r <= (unsigned)(H + 1) && (unsigned)q <= (unsigned)(W + 1)) ? sm[r * BW + q] : 0u;
    };
    auto at = [&](int t) -> uint32_t {
      const int i = t / RB, rem = t - i * RB, j = P > 1 ? rem >> 1 : rem, c = rem - j * P;
      return cell(top + i, left + j, c);
    };
    for (int t = g.row; t < head; t += LPE) dst[t] = (uint8_t)at(t);
    for (int t = tail + g.row; t < T; t += LPE) dst[t] = (uint8_t)at(t);
    for (int k = g.row; k < nch; k += LPE) {
      const int t0 = head + 16 * k;
      const int i = t0 / RB, rem = t0 - i * RB;
      int q = P > 1 ? rem >> 1 : rem;
      int c = rem - q * P, r = top + i;
      q += left;
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int n = 0; n < 16; n++) {
        w[n >> 2] |= cell(r, q, c) << (8 * (n & 3));
        if (++c == P) {
          c = 0;
          if (++q == left + OW) {
            q = left;
            ++r;
          }
        }
      }
      put(t0, w[0], w[1], w[2], w[3]);
    }
  }
}

// one-hot -> codes, one thread per cell (grid-stride): the index of the set byte among the first CS, then the C - CS extra
// bytes as they are
// (four-byte cells -- the 3-D maze, binary with the static plane -- from 4-byte aligned rows: one dword load per cell)
__global__ __launch_bounds__(256) void onehot_to_codes_kernel(const uint8_t *__restrict__ oh, int64_t n_cells, int cells, int C,
                                                              int CS, uint8_t *__restrict__ codes) {
  const int P = 1 + C - CS;
  if (C == 4 && ((uintptr_t)oh & 3u) == 0) {
    const uint32_t *oh4 = (const uint32_t *)oh;
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_cells; x += (int64_t)gridDim.x * blockDim.x) {
      const uint32_t w = oh4[x];  // bytes are 0 / 1
      uint32_t v = 0;
      for (int k = 1; k < CS; k++) v += ((w >> (8 * k)) & 1u) * (uint32_t)k;
      uint8_t *d = codes + x * P;
      d[0] = (uint8_t)v;
      if (P > 1) d[1] = (uint8_t)(w >> 24);
    }
    return;
  }
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_cells; x += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t *src = oh + x * C;
    uint32_t v = 0;
    for (int k = 1; k < CS; k++) v += src[k] ? (uint32_t)k : 0u;
    uint8_t *d = codes + x * P;
    d[0] = (uint8_t)v;
    for (int k = CS; k < C; k++) d[1 + k - CS] = src[k];
  }
}

template <int PROB, int LPE, typename M>
static hipError_t launch_codes_pl(const Params &p, const CodesArgs &a, size_t lds, hipStream_t s) {
  constexpr int EPW = 64 / LPE;
  if (a.rs > 0)
    hipLaunchKernelGGL((codes_observe_kernel<PROB, LPE, M, true>), dim3((p.n_envs + EPW - 1) / EPW), dim3(64), lds, s, p, a);
  else
    hipLaunchKernelGGL((codes_observe_kernel<PROB, LPE, M, false>), dim3((p.n_envs + EPW - 1) / EPW), dim3(64), lds, s, p, a);
  return hipGetLastError();
}

template <int PROB>
static hipError_t launch_codes_prob(const Params &p, int lpe, const CodesArgs &a, size_t lds, hipStream_t s) {
  if (p.cfg.dims[1] > 32) {  // 64-bit row masks: 32 or 64 lanes per env (validate())
    if (lpe == 32) return launch_codes_pl<PROB, 32, uint64_t>(p, a, lds, s);
    return launch_codes_pl<PROB, 64, uint64_t>(p, a, lds, s);
  }
  switch (lpe) {
    case 8: return launch_codes_pl<PROB, 8, uint32_t>(p, a, lds, s);
    case 16: return launch_codes_pl<PROB, 16, uint32_t>(p, a, lds, s);
    case 32: return launch_codes_pl<PROB, 32, uint32_t>(p, a, lds, s);
    default: return launch_codes_pl<PROB, 64, uint32_t>(p, a, lds, s);
  }
}

hipError_t launch_codes_observe(const Params &p, int lpe, const CodesArgs &args, hipStream_t s) {
  CodesArgs a = args;
  const int H = p.cfg.dims[0], W = p.cfg.dims[1], OW = p.cfg.obs_window[1], epw = 64 / lpe;
  // padded rows: window column j of an env at column pos1 is padded index PADL + pos1 - OW / 2 + j; a chunk reads up to 19
  // bytes from its 4-byte aligned start
  a.pad_l = a.wide ? 0 : ((OW / 2 + 3) & ~3);
  const int rs = ((a.wide ? W + 4 : a.pad_l + W + (OW - OW / 2) + 4) + 15) & ~15;
  const size_t pad_lds = (size_t)epw * H * rs + rs;
  a.rs = (a.P == 1 && pad_lds <= 48 * 1024) ? rs : 0;
  a.pre = (a.rs > 0 && p.cfg.problem == PCGRL_PROB_BINARY && !a.wide && !p.ext && H == 16 && W == 16 && lpe == 16 &&
           p.cfg.obs_window[0] == 32 && OW == 32) ? 1 : 0;
  // generic: <= 8.5 KB per workgroup (64 x 64 with static tiles)
  const size_t lds = a.rs > 0 ? pad_lds : ((size_t)H * W + (a.P > 1 ? (size_t)(H + 2) * (W + 2) : 0) + 15) / 16 * 16 * epw;
  switch (p.cfg.problem) {
    case PCGRL_PROB_BINARY: return launch_codes_prob<PCGRL_PROB_BINARY>(p, lpe, a, lds, s);
    case PCGRL_PROB_ZELDA: return launch_codes_prob<PCGRL_PROB_ZELDA>(p, lpe, a, lds, s);
    case PCGRL_PROB_SOKOBAN: return launch_codes_prob<PCGRL_PROB_SOKOBAN>(p, lpe, a, lds, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_onehot_to_codes(const uint8_t *onehot, int64_t n_rows, int cells, int C, int CS, uint8_t *codes, hipStream_t s) {
  const int64_t n = n_rows * (int64_t)cells;
  if (n <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 256 * 32);  // (grid-stride beyond 32 workgroups per CU)
  hipLaunchKernelGGL(onehot_to_codes_kernel, dim3((unsigned)blocks), dim3(256), 0, s, onehot, n, cells, C, CS, codes);
  return hipGetLastError();
}

}  // namespace pcgrl
