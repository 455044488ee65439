// pcgrl_k_step16.hip -- pcgrl::step16_kernel: one step of binary 16x16 envs (narrow / turtle, 32x32 window, plain mode).
//
// The same work as step_kernel<PCGRL_PROB_BINARY, 16, uint32_t, /*FAST=*/true, /*CTRL=*/false, 2> (pcgrl_kernels2d.h), bit for
// bit, on the same state layout and with the same launch geometry; see pcgrl_step16.h for what differs.  Everything that is
// not named *16 here is pcgrl_kernels2d.h's.
#include "pcgrl_step16.h"

#include "../pcgrl_kernels2d.h"

namespace pcgrl {

// (the development counters of PHASE_* / TRACE_* are indexed by workgroup: one wave pair per workgroup in those builds)
#if defined(PCGRL_PHASE_TIMING) || defined(PCGRL_WAVE_TRACE)
constexpr int STEP16_PAIRS = 1;
#else
constexpr int STEP16_PAIRS = 2;
#endif

typedef uint4 __attribute__((may_alias)) uint4_rec;  // the env record as 16-byte words
typedef uint2 __attribute__((may_alias)) uint2_rec;

// SWEEP_UNROLL = 6 levels of bfs_level's 16-lane form as ONE asm statement (f0 -> f1 .. f6, each removed from `fr`).  Between
// two bfs_level statements the compiler has to assume the worst about the hazards at their edges and puts a wait state
// there; inside one statement the order is known: a frontier is read through DPP three instructions after it was written.
#define STEP16_LEVEL(in, out)                                                              \
  "v_lshlrev_b32 %6, 1, " in "\n\t"                                                        \
  "v_lshrrev_b32 %7, 1, " in "\n\t"                                                        \
  "v_or_b32_dpp %6, " in ", %6 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"      \
  "v_or_b32_dpp %7, " in ", %7 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"      \
  "v_bitop3_b32 " out ", %6, %7, %8 bitop3:0xa8\n\t"                                       \
  "v_bitop3_b32 %8, %6, %7, %8 bitop3:2\n\t"
__device__ __attribute__((always_inline)) inline void trip16(uint32_t f0, uint32_t &f1, uint32_t &f2, uint32_t &f3, uint32_t &f4,
                                                             uint32_t &f5, uint32_t &f6, uint32_t &fr) {
  uint32_t a, b;
  asm(STEP16_LEVEL("%9", "%0") STEP16_LEVEL("%0", "%1") STEP16_LEVEL("%1", "%2") STEP16_LEVEL("%2", "%3")
          STEP16_LEVEL("%3", "%4") STEP16_LEVEL("%4", "%5")
      : "=&v"(f1), "=&v"(f2), "=&v"(f3), "=&v"(f4), "=&v"(f5), "=&v"(f6), "=&v"(a), "=&v"(b), "+v"(fr)
      : "v"(f0));
}
#undef STEP16_LEVEL

// sweep() for 16 lanes per env and 32-bit masks, without tracked levels.  Every trip runs its SWEEP_UNROLL levels bare.  A
// group's frontier dies in exactly one trip (a dead frontier stays dead); the frontiers of that trip -- the level it entered
// the trip with and the first SWEEP_UNROLL - 1 it produced, the last one being empty -- are kept in k[], and its level count
// at the trip's start in `base`.  Frontiers are non-empty up to the last level and empty from there on, so the group's
// length is base + the highest index of a non-empty k[], and `last` is that k[].  len, last and visited are sweep()'s:
// len = number of levels, last = the cells of level len (none when len == 0), visited = everything reached.
// Which groups are alive is scalar work on the trip's ballot: bit 15 of a group's 16-bit slice stands for "the slice is not
// zero" ((x & 0x7fff) + 0x7fff carries into bit 15 iff a low bit is set; no carry leaves the slice).
__device__ __attribute__((always_inline)) inline void sweep16(const Grp<16> &g, uint32_t src, uint32_t avail, int &len,
                                                              uint32_t &last, uint32_t &visited) {
  static_assert(SWEEP_UNROLL == 6, "sweep16 keeps six frontiers per trip");
  constexpr uint64_t LOW = 0x7FFF7FFF7FFF7FFFull, TOP = 0x8000800080008000ull;
  uint32_t front = src & avail;
  uint32_t free_cells = avail & ~front;
  // (a group without a source "dies" in the first trip with six empty frontiers: len 0)
  uint32_t k0 = 0, k1 = 0, k2 = 0, k3 = 0, k4 = 0, k5 = 0;
  int base = 0, lev = 0;
  uint64_t alive = TOP;
  while (true) {
    const uint32_t f0 = front;
    uint32_t f1, f2, f3, f4, f5;
    trip16(f0, f1, f2, f3, f4, f5, front, free_cells);
    const uint64_t bal = __ballot(front != 0);
    const uint64_t now = (((bal & LOW) + LOW) | bal) & TOP;
    const uint64_t gone = alive & ~now;
    if (gone != 0) {  // (wave-uniform; at most once per group and sweep)
      const bool died = ((gone >> (g.gbase + 15)) & 1ull) != 0;
      k0 = died ? f0 : k0;
      k1 = died ? f1 : k1;
      k2 = died ? f2 : k2;
      k3 = died ? f3 : k3;
      k4 = died ? f4 : k4;
      k5 = died ? f5 : k5;
      base = died ? lev : base;
    }
    lev += SWEEP_UNROLL;
    alive = now;
    if (now == 0) break;
  }
  int myidx = k1 ? 1 : 0;
  myidx = k2 ? 2 : myidx;
  myidx = k3 ? 3 : myidx;
  myidx = k4 ? 4 : myidx;
  myidx = k5 ? 5 : myidx;
  const int gidx = (int)g.gmax((uint32_t)myidx);
  len = base + gidx;
  uint32_t l = k0;
  l = gidx == 1 ? k1 : l;
  l = gidx == 2 ? k2 : l;
  l = gidx == 3 ? k3 : l;
  l = gidx == 4 ? k4 : l;
  l = gidx == 5 ? k5 : l;
  last = len > 0 ? l : 0u;
  visited = avail & ~free_cells;
}

// component_fars() on sweep16
__device__ inline uint32_t component_fars16(const Grp<16> &g, uint32_t comps) {
  const uint32_t iso = comps & ~expand(g, comps);
  uint32_t remaining = comps & ~iso, fars = iso;
  while (true) {
    const uint64_t gb = g.gballot(remaining != 0);
    if (__ballot(gb != 0) == 0) break;
    const int fl = gb ? __builtin_ctzll(gb) : -1;
    const uint32_t seed = g.row == fl ? (remaining & (0u - remaining)) : 0u;
    int depth;
    uint32_t last, vis;
    sweep16(g, seed, remaining, depth, last, vis);
    fars |= first_rowmajor(g, last);
    remaining &= ~vis;
  }
  return fars;
}

// binary_stats_update() on sweep16: the statistics after editing the single cell `x`
__device__ inline void binary_stats_update16(const Grp<16> &g, uint32_t x, uint32_t p_old, uint32_t p_new, int &regions,
                                             int &path_len, uint32_t &fars, uint32_t &best PHASE_ARG, bool have_pre, uint32_t pre) {
  const bool became_pass = g.gany((x & p_new) != 0);
  const bool edited = g.gany(x != 0);
  uint32_t K = edited ? pre : 0u;
  if (__ballot(edited && !have_pre) != 0) {
    const uint32_t Kf = flood(g, x, became_pass ? p_new : p_old);
    K = have_pre ? K : Kf;
  }
  K = became_pass ? K : (K & ~x);
  const uint32_t touched = K | x;
  const bool hit = g.gany((best & touched) != 0);
  PHASE_MARK(3);  // flood
  const uint32_t newfars = component_fars16(g, K);
  PHASE_MARK(4);  // first sweeps
  fars = (fars & ~touched) | newfars;
  int l;
  uint32_t b, vis;
  sweep16(g, hit ? fars : newfars, p_new, l, b, vis);
  PHASE_MARK(5);  // second sweep
  if (edited) {
    regions = (int)g.gsum((uint32_t)popc_m(fars));
    if (hit || l > path_len) {
      path_len = l;
      best = b;
    }
  } else {
    (void)g.gsum(0u);  // keep the cross-lane reduction in uniform control flow
  }
}

// One workgroup = STEP16_PAIRS x (simulate wave, observe wave) over four envs each, as in step_kernel.  The role is decided
// first; each role asks for all it needs of the old state in one batch and then meets the other at the barrier (the simulate
// wave overwrites that state at its end).
__global__ __launch_bounds__(128 * STEP16_PAIRS, PCGRL_STEP_WAVES) void step16_kernel(Params p) {
  constexpr int PROB = PCGRL_PROB_BINARY, LPE = 16, NS = 2, EPW = 4;
  typedef uint32_t M;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_all[];
  touch_kernarg(p);
  Grp<LPE> g;
  g.init();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int pair = wave >> 1;
  const bool observer = (wave & 1) != 0;  // wave-uniform
  uint8_t *lds = lds_all + (size_t)pair * p.lds_pair_bytes;
  const int env = (int)((blockIdx.x * STEP16_PAIRS + pair) * EPW + (g.lane / LPE));
  const bool active = env < p.n_envs;  // (16 rows on 16 lanes: every lane of an active env owns a row)
  const M colmask = active ? 0xFFFFu : 0u;
  const int e = active ? env : 0;
  M *pl = (M *)p.planes + (size_t)e * ROW_WORDS * 16 + g.row;  // plane k of this lane's row: pl[16 * k]
  EnvState *S = &p.st[e];
  uint64_t *rng_stash = (uint64_t *)(lds + p.lds_pair_bytes - 64 * EPW) + 8 * (g.lane / LPE);

  if (observer) {
    // ---- observe: the tile plane, pos / n_step, iteration / changes, the action; the RNG streams when a reset may come
    TRACE_DECL();
    M b[1];
    b[0] = active ? pl[0] : M(0);
    const uint4 s0 = *(const uint4_rec *)S;                    // pos[0..2], n_step
    const uint2 s1 = *(const uint2_rec *)&S->iteration;        // iteration, changes
    const int action = active ? p.actions[e] : 0;
    // (an auto-reset of this step replays the env's RNG streams here, too; the simulate wave stores the advanced streams at
    // its end.  Asked for with everything else, not after `iteration` has arrived; it waits in LDS behind the pair's rows.)
    if (p.auto_reset != 0 && g.row < 8) rng_stash[g.row] = ((const uint64_t *)&p.rng[e])[g.row];  // rep[4], prob[4]
    __syncthreads();
    int pos[2] = {(int)s0.x, (int)s0.y};
    int n_step = (int)s0.w, iteration = (int)s1.x + 1, changes = (int)s1.y;
    bool bad = false;
    const bool change = rep_update<PROB, LPE, M, true>(g, p, active, action, b, pos, n_step, bad);
    changes += change ? 1 : 0;
    bool done = iteration > p.cfg.max_iterations;
    if (p.cfg.max_changes >= 0) done = done || changes > p.cfg.max_changes;
    const bool do_reset = active && done && p.auto_reset != 0;
    if (__ballot(do_reset) != 0) {
      Pcg obs_rp, obs_rr;
      obs_rr.load(rng_stash);
      obs_rp.load(rng_stash + 4);
      reset_from_rng<PROB, LPE, M>(g, p, e, do_reset, b, pos, /*commit=*/false, nullptr, &obs_rp, &obs_rr);
    }
    encode_obs_any<PROB, LPE, true, M>(g, p, e, active, b, pos, lds);
    // PREFLOOD: the component of the next edit's cell, flooded ahead of time for the next launch's simulate wave
    const M xbit = (active && g.row == pos[0]) ? (M(1) << pos[1]) : M(0);
    const M comp = flood(g, xbit, (~b[0] & colmask) | xbit);
    if (active) pl[16 * PRE_PLANE] = comp | (M)PRE_VALID;
    TRACE_PUT(2, _tr0);
    TRACE_PUT(3, TRACE_NOW());
    TRACE_DRAIN();
    TRACE_PUT(4, TRACE_NOW());
    return;
  }

  // ---- simulate: three planes, the PREFLOOD word, the hot part of the env record, the action
  if (p.n_envs <= 8192) __builtin_amdgcn_s_setprio(3);  // (as in step_kernel: ahead of the observe wave at small batches)
  PHASE_DECL();
  TRACE_DECL();
  M b[3];
  b[0] = active ? pl[0] : M(0);
  b[1] = active ? pl[16] : M(0);
  b[2] = active ? pl[32] : M(0);
  const M pre3 = active ? pl[16 * PRE_PLANE] : M(0);
  const uint4 s0 = ((const uint4_rec *)S)[0];  // pos[0..2], n_step
  const uint4 s1 = ((const uint4_rec *)S)[1];  // iteration, changes, flags, last_ep_len
  const uint4 s2 = ((const uint4_rec *)S)[2];  // last_loss, ep_return
  const uint2 s4 = *(const uint2_rec *)&S->stats[0];
  const int action = active ? p.actions[e] : 0;
  static_assert(offsetof(EnvState, n_step) == 12 && offsetof(EnvState, iteration) == 16 && offsetof(EnvState, last_ep_len) == 28 &&
                    offsetof(EnvState, last_loss) == 32 && offsetof(EnvState, ep_return) == 40 && offsetof(EnvState, stats) == 64,
                "step16_kernel reads and writes the hot line of EnvState as 16-byte words");
  __syncthreads();  // both waves hold the old state before this one may overwrite it
  PHASE_MARK(0);    // loads + barrier
  int pos[2] = {(int)s0.x, (int)s0.y};
  const uint32_t pos2 = s0.z;
  int n_step = (int)s0.w, iteration = (int)s1.x + 1, changes = (int)s1.y, flags = (int)s1.z;
  uint32_t last_ep_len = s1.w;
  double last_loss = __hiloint2double((int)s2.y, (int)s2.x), ep_return = __hiloint2double((int)s2.w, (int)s2.z);
  int32_t st[NS] = {(int32_t)s4.x, (int32_t)s4.y};
  const M tile0_old = b[0];

  // envs/pcgrl_env.py:267-342
  bool bad = false;
  const bool change = rep_update<PROB, LPE, M, true>(g, p, active, action, b, pos, n_step, bad);
  changes += change ? 1 : 0;
  bool done = iteration > p.cfg.max_iterations;
  if (p.cfg.max_changes >= 0) done = done || changes > p.cfg.max_changes;
  const bool do_reset = active && done && p.auto_reset != 0;
  if (bad && g.row == 0 && active) atomicOr(p.err, 1);
  PHASE_MARK(1);  // action
  // a captured launch replayed after pcgrl_update lands here with stale statistics: error bit 8 (see step_kernel)
  if ((flags & ENV_STATS_DIRTY) != 0 && change && active && g.row == 0) atomicOr(p.err, 8);
  if (__ballot(change) != 0) {
    // incremental: only the component(s) touching the edited cell are re-swept
    const M x = change ? (tile0_old ^ b[0]) & colmask : M(0);
    int reg = st[0], len = st[1];
    M fars = b[1], best = b[2];
    binary_stats_update16(g, x, ~tile0_old & colmask, ~b[0] & colmask, reg, len, fars, best PHASE_PASS,
                          g.gany((pre3 & (M)PRE_VALID) != 0), pre3 & colmask);
    if (change) {
      st[0] = reg;
      st[1] = len;
      b[1] = fars;
      b[2] = best;
    }
  }
  PHASE_MARK(2);  // rest of the stats refresh
  // control_wrappers.py:216-244
  const double loss = get_loss<NS>(p, st);
  const double rew = loss - last_loss;
  last_loss = loss;
  ep_return += rew;
  if (active && g.row == 0) {
    if (p.reward) p.reward[e] = (float)rew;
    if (p.done) p.done[e] = done ? 1 : 0;
    if (p.stats_out) {
      p.stats_out[(size_t)e * NS] = st[0];
      p.stats_out[(size_t)e * NS + 1] = st[1];
    }
  }
  if (__ballot(do_reset) != 0) {
    if (do_reset) last_ep_len = (uint32_t)iteration;  // (what latch_episode stores; the record's word is written back below)
    if (do_reset && g.row == 0) latch_episode<NS>(p, e, S, ep_return, iteration, st);
    reset_from_rng<PROB, LPE, M>(g, p, e, do_reset, b, pos, /*commit=*/true, nullptr);
    int32_t ns[NS];
    compute_stats<PROB, LPE, M, false>(g, p, e, do_reset, b, colmask, ns);
    if (do_reset) {
      st[0] = ns[0];
      st[1] = ns[1];
      iteration = 0;
      changes = 0;
      n_step = 0;
      flags = 0;
      ep_return = 0.0;
      last_loss = get_loss<NS>(p, st);
    }
  }
  // write back state
  if ((change || do_reset) && active) {
    pl[0] = b[0];
    pl[16] = b[1];
    pl[32] = b[2];
  }
  if (active && g.row == 0) {
    ((uint4_rec *)S)[0] = make_uint4((uint32_t)pos[0], (uint32_t)pos[1], pos2, (uint32_t)n_step);
    ((uint4_rec *)S)[1] = make_uint4((uint32_t)iteration, (uint32_t)changes, (uint32_t)flags, last_ep_len);
    ((uint4_rec *)S)[2] = make_uint4((uint32_t)__double2loint(last_loss), (uint32_t)__double2hiint(last_loss),
                                     (uint32_t)__double2loint(ep_return), (uint32_t)__double2hiint(ep_return));
    *(uint2_rec *)&S->stats[0] = make_uint2((uint32_t)st[0], (uint32_t)st[1]);
    if (do_reset) accumulate_episode<NS>(S);
  }
  PHASE_MARK(6);  // loss, outputs, write-back
  PHASE_FLUSH();
  TRACE_PUT(0, _tr0);
  TRACE_PUT(1, TRACE_NOW());
}

hipError_t launch_step16(const Params &p, size_t lds, hipStream_t s) {
  const unsigned pairs = (unsigned)((p.n_envs + 3) / 4);
  const dim3 grid((pairs + STEP16_PAIRS - 1) / STEP16_PAIRS);
  hipLaunchKernelGGL(step16_kernel, grid, dim3(128 * STEP16_PAIRS), STEP16_PAIRS * lds, s, p);
  return hipGetLastError();
}

}  // namespace pcgrl
