// multiagent/pcgrl_multiagent.h -- multi-agent turtle stepping on the device (include/pcgrl_amd_multiagent.h): the
// reference's MultiAgentWrapper over MultiAgentTurtleRepresentation, optionally under ShowAgentRepresentation
// (wrappers.py:697-736, reps/wrappers.py:189-231, :616-651), for the binary and zelda problems.
//
// The rules (A agents, positions are (row, col)):
//   reset     the wrapped turtle reset (two doubles for its unused position, then the map), then the spawn draw from the
//             representation's generator: Generator.choice(n_cells, size=A, replace=False) = Floyd's algorithm (for j = n - A
//             .. n - 1: v in [0, j], no draw at j == 0; v = j if v is taken) and a shuffle (for i = A - 1 .. 1: swap i with a
//             draw from [0, i]); every bounded draw is Lemire's method on 32-bit halves of PCG64 draws (pcg_integers), and
//             the unused half is kept from one reset to the next.  n_cells < A: the draw is choice(A, A) and everybody
//             stands on cell 0.
//   round     the agents in index order; agent i absent (action -1) or done since the reset: no sub-step.  A sub-step is a
//             whole PcgrlEnv.step from the agent's own position: iteration + 1, the turtle update, changes + 1 and new
//             statistics if the map changed, reward = the change of the loss, done = iteration > max_iterations or
//             changes > max_changes, and the agent's observation: the crop around its new position of the map as it is
//             right then.  The round after which every agent is done ends the episode.
//   occupancy one more channel behind the one-hot ones: 1 on the cells that hold an agent, cropped like the map.
//
// ma_step_kernel runs ONE ROUND PER LAUNCH with the engine's mapping (LPE lanes per env, one lane per map row, row masks in
// VGPRs) and the two specialised waves of step_kernel / rollout_kernel: wave 0 simulates (statistics, rewards, the state
// write-back), wave 1 replays the A cheap representation updates -- and with them the counters and done bits, which do not
// depend on the statistics -- on its own registers and encodes the A observations, so the searches and the observation
// stores overlap.  The env state stays in registers across the sub-steps.  Lane i of an env's group keeps the position and
// the action of agent i (a group has at least 8 lanes, an env at most 8 agents); a sub-step fetches them with a broadcast,
// so nothing is indexed at run time and nothing spills.
// The per-env side state has arrays of its own (MaArgs): EnvState and Params are as they were.
#pragma once
#include <hip/hip_runtime.h>

#include "../pcgrl_common.h"

namespace pcgrl {

struct MaArgs {
  int32_t n_agents, show_agents;
  int32_t obs_chunks;    // show_agents: 16-byte chunks of one observation row of NT + 2 channels
  int32_t pad_;
  int32_t *pos;          // [N][A][2] (row, col)
  uint32_t *side;        // [N][4]: done bits since the reset, spare-half flag, spare half, 0
  int32_t *last_stats;   // [N][A][PCGRL_MAX_STATS]: the statistics after the agent's last sub-step (after the reset: the reset's)
  const int32_t *init_pos;  // reset with injected maps, pcgrl_ma_set_state: [N][A][2]
  const uint32_t *in_side;  // pcgrl_ma_set_state: [N][4], or null
  const int32_t *in_stats;  // pcgrl_ma_set_state: [N][A][PCGRL_MAX_STATS], or null
  uint8_t *done_all;     // step: [N]
};

enum MaKernel { MA_RESET, MA_STEP, MA_OBSERVE, MA_SET_STATE };

// one per translation unit (the six (LPE, M) forms validate() can choose)
hipError_t launch_ma_binary(MaKernel k, const Params &p, int lpe, const MaArgs &a, size_t lds, hipStream_t s);
hipError_t launch_ma_zelda(MaKernel k, const Params &p, int lpe, const MaArgs &a, size_t lds, hipStream_t s);

inline hipError_t launch_ma(MaKernel k, const Params &p, int lpe, const MaArgs &a, size_t lds, hipStream_t s) {
  switch (p.cfg.problem) {
    case PCGRL_PROB_BINARY: return launch_ma_binary(k, p, lpe, a, lds, s);
    case PCGRL_PROB_ZELDA: return launch_ma_zelda(k, p, lpe, a, lds, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace pcgrl

#ifdef PCGRL_KERNEL_TU
#include "../pcgrl_kernels2d.h"

namespace pcgrl {

__device__ inline uint32_t ma_pack(int r, int c) { return (uint32_t)r | ((uint32_t)c << 16); }

// the spawn draw; every lane of the group replays it, lane k keeps the cell of agent k; only `on` groups take the result
template <int LPE>
__device__ inline void ma_spawn(const Grp<LPE> &g, int n_cells, int W, int A, bool on, Pcg &rr, uint32_t &has32, uint32_t &val32,
                                uint32_t &mypos) {
  Pcg r = rr;
  uint32_t h = has32, v32 = val32;
  const bool crowded = n_cells < A;
  const int n = crowded ? A : n_cells;
  uint32_t mine = 0xFFFFFFFFu;
  for (int k = 0; k < A; k++) {
    const int j = n - A + k;
    uint32_t v = (uint32_t)pcg_integers(r, h, v32, 0, j + 1);
    if (g.gany(g.row < k && mine == v)) v = (uint32_t)j;
    mine = g.row == k ? v : mine;
  }
  for (int i = A - 1; i >= 1; i--) {
    const int j = pcg_integers(r, h, v32, 0, i + 1);
    const uint32_t vi = g.gbcast(mine, i), vj = g.gbcast(mine, j);
    mine = g.row == i ? vj : (g.row == j ? vi : mine);
  }
  if (on) {
    rr = r;
    has32 = h;
    val32 = v32;
    if (g.row < A) {
      const int cell = crowded ? 0 : (int)mine;
      const int rw = cell / W;
      mypos = ma_pack(rw, cell - rw * W);
    }
  }
}

// Observation with the agent_occupancy plane: C = NT + 2 channels (out of bounds, the tiles, occupancy).  The plane has the
// map's shape and goes through the same crop, so it is zero outside the map.  As in encode_obs every lane builds the
// observation row of its map row in LDS (LDS row 64: the all-out-of-bounds row) and the group streams the window out.
template <int PROB, int LPE, typename M>
__device__ inline void encode_obs_agents(const Grp<LPE> &g, const Params &p, int CH, int slot, bool active, const M *b,
                                         const int *pos, M occ, uint8_t *lds) {
  constexpr int NT = ProbTraits<PROB>::NT, NB = ProbTraits<PROB>::NB, C = NT + 2;
  const int H = p.cfg.dims[0], W = p.cfg.dims[1], OH = p.cfg.obs_window[0], OW = p.cfg.obs_window[1];
  const int RB = OW * C, STRIDE = CH * 16 + 16;
  const int top = pos[0] - OH / 2, left = pos[1] - OW / 2;
  uint8_t *row = lds + g.lane * STRIDE;
  uint8_t *oob_row = lds + 64 * STRIDE;
  for (int q = 0; q < CH; q++) *(uint4 *)(row + q * 16) = make_uint4(0, 0, 0, 0);
  for (int q = g.lane; q < CH; q += 64) *(uint4 *)(oob_row + q * 16) = make_uint4(0, 0, 0, 0);
  if (g.row < H) {
    for (int j = 0; j < OW; j++) {
      const int q = left + j;
      uint8_t *px = row + j * C;
      if (q >= 0 && q < W) {
        px[1 + tile_at<NB, M>(b, q)] = 1;
        px[C - 1] = (uint8_t)((occ >> q) & M(1));
      } else {
        px[0] = 1;
      }
    }
  }
  for (int j = g.lane; j < OW; j += 64) oob_row[j * C] = 1;
  if (active) {
    uint8_t *base = p.obs + (size_t)slot * OH * RB;
    const int gb = g.gbase;
    if (RB & 15) {
      stream_obs_bytes(g, base, OH, RB, [&](int i) -> const uint8_t * {
        const int m = i + top;
        return (unsigned)m < (unsigned)H ? lds + (gb + m) * STRIDE : oob_row;
      });
    } else {
      stream_obs_chunks(g, base, OH * CH, CH, [&](int i) -> const uint8_t * {
        const int m = i + top;
        return (unsigned)m < (unsigned)H ? lds + (gb + m) * STRIDE : oob_row;
      });
    }
  }
}

// the observation of one agent into slot [env][agent]; mypos: lane k of the group holds agent k's position
template <int PROB, int LPE, typename M>
__device__ inline void ma_encode(const Grp<LPE> &g, const Params &p, const MaArgs &a, int slot, bool active, const M *b,
                                 const int *pos, uint32_t mypos, uint8_t *lds) {
  if (!a.show_agents) {
    // (the general encoder also on a 16x16 map with a 32x32 window: encode_obs_any's compile-time encoder next to it inside
    // the agent loop takes the (16, 32) form past 256 registers, to one wave per SIMD -- DESIGN.md section 15)
    encode_obs<PROB, LPE, false, M, false>(g, p, slot, active, b, pos, lds, p.obs);
    return;
  }
  M occ = M(0);
  for (int i = 0; i < a.n_agents; i++) {
    const uint32_t v = g.gbcast(mypos, i);
    occ |= (int)(v & 0xFFFFu) == g.row ? (M(1) << (v >> 16)) : M(0);
  }
  encode_obs_agents<PROB, LPE, M>(g, p, a.obs_chunks, slot, active, b, pos, occ, lds);
}

// One round of every env.  Wave 0 simulates, wave 1 observes (see the head of this file).
template <int PROB, int LPE, typename M>
__global__ __launch_bounds__(128) void ma_step_kernel(Params p, MaArgs a) {
  constexpr int NB = ProbTraits<PROB>::NB, NS = ProbTraits<PROB>::NS, EPW = 64 / LPE;
  constexpr int NW = NB + ProbTraits<PROB>::NAUX;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  Grp<LPE> g;
  g.init();
  const bool observer = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) != 0;  // wave-uniform
  if (observer && p.obs == nullptr) return;
  PHASE_DECL();
  const int H = p.cfg.dims[0], W = p.cfg.dims[1], A = a.n_agents;
  const int env = blockIdx.x * EPW + (g.lane / LPE);
  const bool active = env < p.n_envs;
  const bool rowok = active && g.row < H;
  const M colmask = rowok ? (W >= (int)(8 * sizeof(M)) ? ~M(0) : ((M(1) << W) - M(1))) : M(0);
  const int e = active ? env : 0;

  // both waves take the whole state before wave 0 may overwrite any of it
  M b[NW];
  load_planes<NW, M>(p, e, g.row, rowok, b);
  EnvState *S = &p.st[e];
  int iteration = S->iteration, changes = S->changes;
  double last_loss = S->last_loss, ep_return = S->ep_return;
  int32_t st[NS];
#pragma unroll
  for (int k = 0; k < NS; k++) st[k] = S->stats[k];
  int tpos[2] = {S->pos[0], S->pos[1]};  // the wrapped turtle's own position: drawn at every reset, never used
  uint32_t *sd = a.side + (size_t)e * 4;
  uint32_t bits = sd[0], has32 = sd[1], val32 = sd[2];
  const bool mine = g.row < A;
  int32_t *mypos_mem = a.pos + ((size_t)e * A + (mine ? g.row : 0)) * 2;
  uint32_t mypos = mine ? ma_pack(mypos_mem[0], mypos_mem[1]) : 0u;
  const int myact = (active && mine) ? p.actions[(size_t)e * A + g.row] : -1;
  Pcg rp, rr;
  rp.load(p.rng[e].prob);
  rr.load(p.rng[e].rep);
  if (p.obs != nullptr) __syncthreads();
  const uint32_t full = (1u << A) - 1u;
  bool any_change = false, bad_any = false;

#pragma nounroll
  for (int i = 0; i < A; i++) {
    const int action = (int)g.gbcast((uint32_t)myact, i);
    const bool present = active && action != -1 && ((bits >> i) & 1u) == 0;
    const uint32_t pv = g.gbcast(mypos, i);
    int pos[2] = {(int)(pv & 0xFFFFu), (int)(pv >> 16)};
    const M tile0_old = b[0];
    M pre[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) pre[k] = b[k];
    bool bad = false;
    int n_step = 0;
    iteration += present ? 1 : 0;
    const bool change = rep_update<PROB, LPE, M>(g, p, present, action, b, pos, n_step, bad);
    bad_any = bad_any || (present && bad);
    changes += change ? 1 : 0;
    bool done = iteration > p.cfg.max_iterations;
    if (p.cfg.max_changes >= 0) done = done || changes > p.cfg.max_changes;
    mypos = g.row == i ? ma_pack(pos[0], pos[1]) : mypos;
    bits |= (present && done) ? (1u << i) : 0u;
    if (observer) {
      ma_encode<PROB, LPE, M>(g, p, a, e * A + i, present, b, pos, mypos, lds);
    } else {
      refresh_stats<PROB, LPE, M, false>(g, p, e, change, false, tile0_old, pre, b, colmask, st PHASE_PASS);
      const double loss = get_loss<NS>(p, st);
      const double rew = present ? loss - last_loss : 0.0;
      if (present) {
        last_loss = loss;
        ep_return += rew;
      }
      if (active && g.row == 0) {
        const size_t o = (size_t)e * A + i;
        int32_t *ls = a.last_stats + o * PCGRL_MAX_STATS;
        if (present) {
#pragma unroll
          for (int k = 0; k < NS; k++) ls[k] = st[k];
        }
        if (p.reward) p.reward[o] = (float)rew;
        if (p.done) p.done[o] = (uint8_t)((bits >> i) & 1u);
        if (p.stats_out) {
#pragma unroll
          for (int k = 0; k < NS; k++) p.stats_out[o * NS + k] = present ? st[k] : ls[k];
        }
      }
      any_change = any_change || change;
    }
  }

  const bool all = active && bits == full;
  const bool do_reset = all && p.auto_reset != 0;
  if (!observer && active && g.row == 0 && a.done_all) a.done_all[e] = all ? 1 : 0;
  if (__ballot(do_reset) != 0) {
    if (!observer && do_reset && g.row == 0) {
      latch_episode<NS>(p, e, S, ep_return, iteration, st);
      accumulate_episode<NS>(S);
    }
    reset_from_rng<PROB, LPE, M>(g, p, e, do_reset, b, tpos, false, nullptr, &rp, &rr);
    ma_spawn(g, p.n_cells, W, A, do_reset, rr, has32, val32, mypos);
    if (do_reset) {
      bits = 0;
      iteration = 0;
      changes = 0;
    }
    if (observer) {
#pragma nounroll
      for (int i = 0; i < A; i++) {  // the first observations of the new episode
        const uint32_t pv = g.gbcast(mypos, i);
        const int pos[2] = {(int)(pv & 0xFFFFu), (int)(pv >> 16)};
        ma_encode<PROB, LPE, M>(g, p, a, e * A + i, do_reset, b, pos, mypos, lds);
      }
    } else {
      int32_t ns[NS];
      compute_stats<PROB, LPE, M, true>(g, p, e, do_reset, b, colmask, ns);
      if (do_reset) {
#pragma unroll
        for (int k = 0; k < NS; k++) st[k] = ns[k];
        ep_return = 0.0;
        last_loss = get_loss<NS>(p, st);
        if (mine) {
          int32_t *ls = a.last_stats + ((size_t)e * A + g.row) * PCGRL_MAX_STATS;
#pragma unroll
          for (int k = 0; k < NS; k++) ls[k] = st[k];
        }
      }
    }
  }
  if (observer) return;
  if (bad_any && g.row == 0) atomicOr(p.err, 1);
  if (any_change || do_reset) store_planes<NW, M>(p, e, g.row, rowok, b);
  if constexpr (PROB == PCGRL_PROB_BINARY) {  // PREFLOOD plane: not maintained here
    if (rowok) ((M *)p.planes)[((size_t)e * ROW_WORDS + PRE_PLANE) * H + g.row] = M(0);
  }
  if (active && mine) {
    mypos_mem[0] = (int32_t)(mypos & 0xFFFFu);
    mypos_mem[1] = (int32_t)(mypos >> 16);
  }
  if (active && g.row == 0) {
    S->pos[0] = tpos[0];
    S->pos[1] = tpos[1];
    S->iteration = iteration;
    S->changes = changes;
    S->last_loss = last_loss;
    S->ep_return = ep_return;
#pragma unroll
    for (int k = 0; k < NS; k++) S->stats[k] = st[k];
    sd[0] = bits;
    sd[1] = has32;
    sd[2] = val32;
    if (do_reset) {
      rr.store(p.rng[e].rep);
      rp.store(p.rng[e].prob);
    }
  }
}

// pcgrl_ma_reset: a new map and the spawn draw from the env's generators, or injected maps with injected positions
template <int PROB, int LPE, typename M>
__global__ __launch_bounds__(64) void ma_reset_kernel(Params p, MaArgs a) {
  constexpr int NB = ProbTraits<PROB>::NB, NS = ProbTraits<PROB>::NS, EPW = 64 / LPE;
  constexpr int NW = NB + ProbTraits<PROB>::NAUX;
  Grp<LPE> g;
  g.init();
  const int H = p.cfg.dims[0], W = p.cfg.dims[1], A = a.n_agents;
  const int env = blockIdx.x * EPW + (g.lane / LPE);
  const bool inb = env < p.n_envs;
  const int e = inb ? env : 0;
  const bool active = inb && (p.mask == nullptr || p.mask[e] != 0);
  const bool rowok = active && g.row < H;
  const M colmask = rowok ? (W >= (int)(8 * sizeof(M)) ? ~M(0) : ((M(1) << W) - M(1))) : M(0);
  const bool mine = g.row < A;
  EnvState *S = &p.st[e];
  uint32_t *sd = a.side + (size_t)e * 4;
  uint32_t has32 = sd[1], val32 = sd[2], mypos = 0u;
  M b[NW];
#pragma unroll
  for (int k = 0; k < NW; k++) b[k] = 0;
  int tpos[2] = {0, 0};
  bool clamped = false;
  if (p.init_grids) {  // injected maps and positions draw nothing
    if (rowok) {
      const uint8_t *src = p.init_grids + ((size_t)e * H + g.row) * W;
      for (int x = 0; x < W; x++) {
        int t = src[x];
        if (t >= ProbTraits<PROB>::NT) {  // no such tile: empty, and the error bit
          t = 0;
          clamped = true;
        }
#pragma unroll
        for (int k = 0; k < NB; k++) b[k] |= (M)((t >> k) & 1) << x;
      }
    }
    if (active && mine) {
      const int32_t *q = a.init_pos + ((size_t)e * A + g.row) * 2;
      const int r = min(max(q[0], 0), H - 1), c = min(max(q[1], 0), W - 1);
      clamped = clamped || r != q[0] || c != q[1];
      mypos = ma_pack(r, c);
    }
  } else {
    Pcg rp, rr;
    rp.load(p.rng[e].prob);
    rr.load(p.rng[e].rep);
    reset_from_rng<PROB, LPE, M>(g, p, e, active, b, tpos, false, nullptr, &rp, &rr);
    ma_spawn(g, p.n_cells, W, A, active, rr, has32, val32, mypos);
    if (active && g.row == 0) {
      rr.store(p.rng[e].rep);
      rp.store(p.rng[e].prob);
    }
  }
  if (clamped) atomicOr(p.err, 1);  // a position outside the map, a tile id outside the problem's
  int32_t st[NS];
  compute_stats<PROB, LPE, M, true>(g, p, e, active, b, colmask, st);
  store_planes<NW, M>(p, e, g.row, rowok, b);
  if constexpr (PROB == PCGRL_PROB_BINARY) {
    if (rowok) ((M *)p.planes)[((size_t)e * ROW_WORDS + PRE_PLANE) * H + g.row] = M(0);
  }
  if (active && mine) {
    int32_t *q = a.pos + ((size_t)e * A + g.row) * 2;
    q[0] = (int32_t)(mypos & 0xFFFFu);
    q[1] = (int32_t)(mypos >> 16);
    int32_t *ls = a.last_stats + ((size_t)e * A + g.row) * PCGRL_MAX_STATS;
#pragma unroll
    for (int k = 0; k < NS; k++) ls[k] = st[k];
  }
  if (active && g.row == 0) {
    S->pos[0] = tpos[0];
    S->pos[1] = tpos[1];
    S->pos[2] = 0;
    S->n_step = 0;
    S->iteration = 0;
    S->changes = 0;
    S->flags = 0;
    S->ep_return = 0.0;
    S->last_loss = get_loss<NS>(p, st);
#pragma unroll
    for (int k = 0; k < NS; k++) S->stats[k] = st[k];
    sd[0] = 0u;
    sd[1] = has32;
    sd[2] = val32;
    sd[3] = 0u;
  }
}

// pcgrl_ma_observe: the A observations of every env's current state
template <int PROB, int LPE, typename M>
__global__ __launch_bounds__(64) void ma_observe_kernel(Params p, MaArgs a) {
  constexpr int NB = ProbTraits<PROB>::NB, EPW = 64 / LPE;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  Grp<LPE> g;
  g.init();
  const int A = a.n_agents;
  const int env = blockIdx.x * EPW + (g.lane / LPE);
  const bool active = env < p.n_envs;
  const int e = active ? env : 0;
  const bool rowok = active && g.row < p.cfg.dims[0];
  M b[NB];
  load_planes<NB, M>(p, e, g.row, rowok, b);
  const int32_t *q = a.pos + ((size_t)e * A + (g.row < A ? g.row : 0)) * 2;
  const uint32_t mypos = g.row < A ? ma_pack(q[0], q[1]) : 0u;
#pragma nounroll
  for (int i = 0; i < A; i++) {
    const uint32_t pv = g.gbcast(mypos, i);
    const int pos[2] = {(int)(pv & 0xFFFFu), (int)(pv >> 16)};
    ma_encode<PROB, LPE, M>(g, p, a, e * A + i, active, b, pos, mypos, lds);
  }
}

// pcgrl_ma_set_state: the caller's side state into the engine's arrays, one thread per (env, agent); positions are clamped to
// the map (the observation encoders index LDS rows by them)
static __global__ __launch_bounds__(64) void ma_set_state_kernel(Params p, MaArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= p.n_envs * a.n_agents) return;
  const int env = i / a.n_agents;
  if (p.mask != nullptr && p.mask[env] == 0) return;
  if (a.init_pos != nullptr) {
    const int r = a.init_pos[2 * (size_t)i], c = a.init_pos[2 * (size_t)i + 1];
    const int rc = min(max(r, 0), p.cfg.dims[0] - 1), cc = min(max(c, 0), p.cfg.dims[1] - 1);
    if (rc != r || cc != c) atomicOr(p.err, 1);
    a.pos[2 * (size_t)i] = rc;
    a.pos[2 * (size_t)i + 1] = cc;
  }
  if (a.in_stats != nullptr)
    for (int k = 0; k < PCGRL_MAX_STATS; k++) a.last_stats[(size_t)i * PCGRL_MAX_STATS + k] = a.in_stats[(size_t)i * PCGRL_MAX_STATS + k];
  if (a.in_side != nullptr && i == env * a.n_agents) {
    const uint32_t full = (1u << a.n_agents) - 1u;
    a.side[(size_t)env * 4 + 0] = a.in_side[(size_t)env * 4 + 0] & full;
    a.side[(size_t)env * 4 + 1] = a.in_side[(size_t)env * 4 + 1] ? 1u : 0u;
    a.side[(size_t)env * 4 + 2] = a.in_side[(size_t)env * 4 + 2];
    a.side[(size_t)env * 4 + 3] = 0u;
  }
}

template <int PROB, int LPE, typename M>
static hipError_t launch_ma_pl(MaKernel k, const Params &p, const MaArgs &a, size_t lds, hipStream_t s) {
  constexpr int EPW = 64 / LPE;
  const dim3 grid((p.n_envs + EPW - 1) / EPW);
  hipError_t e = hipSuccess;
  switch (k) {
    case MA_RESET: hipLaunchKernelGGL((ma_reset_kernel<PROB, LPE, M>), grid, dim3(64), 0, s, p, a); break;
    case MA_STEP:
      // (LDS above the 64 KiB default needs an explicit opt-in per kernel)
      if (lds > 64 * 1024 && (e = hipFuncSetAttribute((const void *)ma_step_kernel<PROB, LPE, M>,
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess)
        return e;
      hipLaunchKernelGGL((ma_step_kernel<PROB, LPE, M>), grid, dim3(128), lds, s, p, a);
      break;
    case MA_OBSERVE:
      if (lds > 64 * 1024 && (e = hipFuncSetAttribute((const void *)ma_observe_kernel<PROB, LPE, M>,
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess)
        return e;
      hipLaunchKernelGGL((ma_observe_kernel<PROB, LPE, M>), grid, dim3(64), lds, s, p, a);
      break;
    case MA_SET_STATE:
      hipLaunchKernelGGL(ma_set_state_kernel, dim3((p.n_envs * a.n_agents + 63) / 64), dim3(64), 0, s, p, a);
      break;
  }
  return hipGetLastError();
}

template <int PROB>
static hipError_t launch_ma_prob(MaKernel k, const Params &p, int lpe, const MaArgs &a, size_t lds, hipStream_t s) {
  if (p.n_envs <= 0) return hipSuccess;
  if (p.cfg.dims[1] > 32) {  // 64-bit row masks: 32 or 64 lanes per env (validate())
    if (lpe == 32) return launch_ma_pl<PROB, 32, uint64_t>(k, p, a, lds, s);
    return launch_ma_pl<PROB, 64, uint64_t>(k, p, a, lds, s);
  }
  switch (lpe) {
    case 8: return launch_ma_pl<PROB, 8, uint32_t>(k, p, a, lds, s);
    case 16: return launch_ma_pl<PROB, 16, uint32_t>(k, p, a, lds, s);
    case 32: return launch_ma_pl<PROB, 32, uint32_t>(k, p, a, lds, s);
    default: return launch_ma_pl<PROB, 64, uint32_t>(k, p, a, lds, s);
  }
}

}  // namespace pcgrl
#endif
