// pcgrl_k_step16.hip -- pcgrl::step16_kernel: one step of binary 16x16 envs (narrow / turtle, 32x32 window, plain mode).
//
// The same work as step_kernel<PCGRL_PROB_BINARY, 16, uint32_t, /*FAST=*/true, /*CTRL=*/false, 2> (pcgrl_kernels2d.h), bit for
// bit, on the same state layout and with the same launch geometry; see pcgrl_step16.h for what differs.  Everything that is
// not named *16 here is pcgrl_kernels2d.h's.  The observe wave's encoder comes in two forms chosen by the batch size
// (encode_obs16_regs up to 8 192 envs, encode_obs16 above); -DPCGRL_STEP16_OBS_REGS=0 builds the unit without the former.
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

// Per-lane constants of the sweeps: functions of the lane index alone.
struct Sweep16Lane {
  uint32_t gbit;   // 1 << (index of the lane's group in the wave): the group's bit in the four-bit alive masks
  uint32_t rkey;   // 15 - row: ends a key, so that the lowest row wins a max-reduction among equal keys
  uint32_t below;  // the rows of the group in front of this one, as bits of the group's ballot slice
  __device__ inline void init(const Grp<16> &g) {
    gbit = 1u << (g.gbase >> 4);
    rkey = 15u - (uint32_t)g.row;
    below = (1u << g.row) - 1u;
  }
};

// sweep() for 16 lanes per env and 32-bit masks, without tracked levels, as one asm statement: the trips, their control and
// the wrap-up.  (Between two statements the compiler has to assume the worst about the hazards at their edges; inside one
// the order is known: a value is read through DPP, or a compare's mask by a select, at least three instructions after it
// was written.)
//
// A trip is SWEEP_UNROLL = 6 levels of bfs_level's 16-lane form.  A group's frontier dies in exactly one trip (a dead
// frontier stays dead; a group without a source dies in the first trip with six empty frontiers); the frontiers of that
// trip -- the level it entered the trip with and the first five it produced, the last one being empty -- are kept in
// k0..k5, and its level count at the trip's start in `base`.  Frontiers are non-empty up to the last level and empty from
// there on, so the group's length is base + the highest index of a non-empty k, and `last` is that k.
//
// Trip control.  vcc = ballot of the trip's last frontier; two s_quadmask fold it to one bit per group (`now`), the groups
// that died in this trip are was & ~now, and the branch to the capture block (off the fall-through path, at most once per
// group and sweep) takes the SCC of that s_andn2.  The loop goes on while vcc != 0.  The body is laid out twice with the two
// frontier registers and the two mask registers swapped, so nothing is copied and one branch is taken per two trips.
// `lev` counts levels in units of 16 (96 per trip): base = lev | rkey, and a lane's key is base + 16 * (1 + the highest
// index of a non-empty k of its own; 0 when it has none).  Keys of a group differ in their last four bits, so ONE
// max-reduction K gives the length ((K >> 4) - 1; a group without any cell has K < 16 and length 0), the lanes that hold
// the last level (same key >> 4: a lane has k[gidx] != 0 exactly when its own highest index is gidx) and the first of them
// in row-major order (key == K); the length is positive exactly when K >= 32.  Each lane has selected its own highest
// non-empty k meanwhile (`b`), which fills the wait states of the reduction.  Every group dies once, so k0..k5 and base
// need no initial value.  (The statements are volatile so that they stay between the PHASE_MARKs of the development builds.)
#define S16_LEVEL(in, out)                                                                   \
  "v_lshlrev_b32 %[a], 1, " in "\n\t"                                                        \
  "v_lshrrev_b32 %[b], 1, " in "\n\t"                                                        \
  "v_or_b32_dpp %[a], " in ", %[a] row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"    \
  "v_or_b32_dpp %[b], " in ", %[b] row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"    \
  "v_bitop3_b32 " out ", %[a], %[b], %[fr] bitop3:0xa8\n\t"                                  \
  "v_bitop3_b32 %[fr], %[a], %[b], %[fr] bitop3:2\n\t"
#define S16_TRIP(in, out, was, now, cap)                                                                           \
  S16_LEVEL(in, "%[t1]") S16_LEVEL("%[t1]", "%[t2]") S16_LEVEL("%[t2]", "%[t3]") S16_LEVEL("%[t3]", "%[t4]")       \
  S16_LEVEL("%[t4]", "%[t5]") S16_LEVEL("%[t5]", out)                                                              \
  "v_cmp_ne_u32 vcc, 0, " out "\n\t"                                                                               \
  "s_quadmask_b64 vcc, vcc\n\t"                                                                                    \
  "s_quadmask_b32 " now ", vcc_lo\n\t"                                                                             \
  "s_andn2_b32 %[gone], " was ", " now "\n\t"                                                                      \
  "s_cbranch_scc1 " cap "\n\t"
#define S16_CAPTURE(in)                                        \
  "v_and_b32 %[a], %[gone], %[gbit]\n\t"                       \
  "v_cmp_ne_u32_e64 %[m1], 0, %[a]\n\t"                        \
  "v_or_b32 %[b], %[lev], %[rkey]\n\t"                         \
  "s_nop 0\n\t"                                                \
  "v_cndmask_b32_e64 %[k0], %[k0], " in ", %[m1]\n\t"          \
  "v_cndmask_b32_e64 %[k1], %[k1], %[t1], %[m1]\n\t"           \
  "v_cndmask_b32_e64 %[k2], %[k2], %[t2], %[m1]\n\t"           \
  "v_cndmask_b32_e64 %[k3], %[k3], %[t3], %[m1]\n\t"           \
  "v_cndmask_b32_e64 %[k4], %[k4], %[t4], %[m1]\n\t"           \
  "v_cndmask_b32_e64 %[k5], %[k5], %[t5], %[m1]\n\t"           \
  "v_cndmask_b32_e64 %[base], %[base], %[b], %[m1]\n\t"
// the loop, then (at .Ls16_done) each lane's key in %[a]; m1..m4 and vcc say which of k1..k5 are non-empty in the lane
#define S16_SWEEP                                                         \
  "s_mov_b32 %[ma], 15\n\t"                                               \
  "s_mov_b32 %[lev], 0\n"                                                 \
  ".Ls16_a%=:\n\t"                                                        \
  S16_TRIP("%[fa]", "%[fb]", "%[ma]", "%[mb]", ".Ls16_cap_a%=")           \
  "\n.Ls16_ra%=:\n\t"                                                     \
  "s_addk_i32 %[lev], 0x60\n\t"                                           \
  "s_cbranch_vccz .Ls16_done%=\n\t"                                       \
  S16_TRIP("%[fb]", "%[fa]", "%[mb]", "%[ma]", ".Ls16_cap_b%=")           \
  "\n.Ls16_rb%=:\n\t"                                                     \
  "s_addk_i32 %[lev], 0x60\n\t"                                           \
  "s_cbranch_vccnz .Ls16_a%=\n\t"                                         \
  "s_branch .Ls16_done%=\n"                                               \
  ".Ls16_cap_a%=:\n\t"                                                    \
  S16_CAPTURE("%[fa]")                                                    \
  "s_branch .Ls16_ra%=\n"                                                 \
  ".Ls16_cap_b%=:\n\t"                                                    \
  S16_CAPTURE("%[fb]")                                                    \
  "s_branch .Ls16_rb%=\n"                                                 \
  ".Ls16_done%=:\n\t"                                                     \
  "v_cmp_ne_u32_e64 %[m1], 0, %[k1]\n\t"                                  \
  "v_cmp_ne_u32_e64 %[m2], 0, %[k2]\n\t"                                  \
  "v_cmp_ne_u32_e64 %[m3], 0, %[k3]\n\t"                                  \
  "v_cmp_ne_u32_e64 %[m4], 0, %[k4]\n\t"                                  \
  "v_cmp_ne_u32 vcc, 0, %[k5]\n\t"                                        \
  "v_min_u32 %[a], 1, %[k0]\n\t"                                          \
  "v_cndmask_b32_e64 %[a], %[a], 2, %[m1]\n\t"                            \
  "v_cndmask_b32_e64 %[a], %[a], 3, %[m2]\n\t"                            \
  "v_cndmask_b32_e64 %[a], %[a], 4, %[m3]\n\t"                            \
  "v_cndmask_b32_e64 %[a], %[a], 5, %[m4]\n\t"                            \
  "v_cndmask_b32_e64 %[a], %[a], 6, vcc\n\t"                              \
  "v_lshl_add_u32 %[a], %[a], 4, %[base]\n\t"
#define S16_OWN(k, m) "v_cndmask_b32_e64 %[b], %[b], " k ", " m "\n\t"
#define S16_MAX(src, ctrl) "v_max_u32_dpp %[t1], " src ", " src " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define S16_SUM(ctrl) "v_add_u32_dpp %[sum], %[sum], %[sum] " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define S16_OPERANDS                                                                                                     \
  [fa] "+v"(fa), [fr] "+v"(free_cells), [fb] "=&v"(fb), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [t4] "=&v"(t4),  \
  [t5] "=&v"(t5), [a] "=&v"(a), [b] "=&v"(b), [k0] "=&v"(k0), [k1] "=&v"(k1), [k2] "=&v"(k2), [k3] "=&v"(k3),            \
  [k4] "=&v"(k4), [k5] "=&v"(k5), [base] "=&v"(base), [ma] "=&s"(ma), [mb] "=&s"(mb), [lev] "=&s"(lev),                  \
  [gone] "=&s"(gone), [m1] "=&s"(m1), [m2] "=&s"(m2), [m3] "=&s"(m3), [m4] "=&s"(m4)

// The sweep from the single cell `seed` of a component_fars16 piece.  free_cells: in, the cells that may still be reached
// (without the seed); out, those that were not.  Returns first_rowmajor(g, last): the first cell in row-major order of the
// last level (none when the sweep has no level at all).
__device__ __attribute__((always_inline)) inline uint32_t sweep16_far(const Sweep16Lane &c, uint32_t seed, uint32_t &free_cells) {
  static_assert(SWEEP_UNROLL == 6, "sweep16 keeps six frontiers per trip");
  uint32_t fa = seed, fb, t1, t2, t3, t4, t5, a, b, k0, k1, k2, k3, k4, k5, base, ma, mb, lev, gone;
  uint64_t m1, m2, m3, m4;
  asm volatile(S16_SWEEP
      "v_cndmask_b32_e64 %[b], %[k0], %[k1], %[m1]\n\t"
      S16_OWN("%[k2]", "%[m2]")
      S16_MAX("%[a]", "quad_perm:[1,0,3,2]")
      S16_OWN("%[k3]", "%[m3]")
      S16_OWN("%[k4]", "%[m4]")
      S16_MAX("%[t1]", "quad_perm:[2,3,0,1]")
      S16_OWN("%[k5]", "vcc")
      "v_sub_u32 %[t2], 0, %[b]\n\t"
      S16_MAX("%[t1]", "row_half_mirror")
      "v_and_b32 %[t2], %[b], %[t2]\n\t"
      "s_nop 0\n\t"
      S16_MAX("%[t1]", "row_mirror")
      "v_cmp_eq_u32_e64 %[m1], %[t1], %[a]\n\t"
      "v_cmp_lt_u32_e64 %[m2], 31, %[t1]\n\t"
      "s_and_b64 %[m1], %[m1], %[m2]\n\t"
      "v_cndmask_b32_e64 %[t3], 0, %[t2], %[m1]"
      : S16_OPERANDS
      : [gbit] "v"(c.gbit), [rkey] "v"(c.rkey)
      : "vcc", "scc");
  return t3;
}

// The sweep from all cells of `src` through `avail`: len = number of levels, last = the cells of level len (none when
// len == 0).  `sum` rides along: in, a value per lane; out, its sum over the group in every lane (gsum's butterfly, whose
// steps and the max-reduction's fill each other's wait states).
__device__ __attribute__((always_inline)) inline void sweep16_len(const Sweep16Lane &c, uint32_t src, uint32_t avail, int &len,
                                                                  uint32_t &last, uint32_t &sum) {
  uint32_t fa = src & avail, free_cells = avail & ~fa;
  uint32_t fb, t1, t2, t3, t4, t5, a, b, k0, k1, k2, k3, k4, k5, base, ma, mb, lev, gone;
  uint64_t m1, m2, m3, m4;
  asm volatile(S16_SWEEP
      "v_cndmask_b32_e64 %[b], %[k0], %[k1], %[m1]\n\t"
      S16_OWN("%[k2]", "%[m2]")
      S16_MAX("%[a]", "quad_perm:[1,0,3,2]")
      S16_SUM("quad_perm:[1,0,3,2]")
      S16_OWN("%[k3]", "%[m3]")
      S16_MAX("%[t1]", "quad_perm:[2,3,0,1]")
      S16_SUM("quad_perm:[2,3,0,1]")
      S16_OWN("%[k4]", "%[m4]")
      S16_MAX("%[t1]", "row_half_mirror")
      S16_SUM("row_half_mirror")
      S16_OWN("%[k5]", "vcc")
      S16_MAX("%[t1]", "row_mirror")
      S16_SUM("row_mirror")
      "v_xor_b32 %[t2], %[t1], %[a]\n\t"
      "v_cmp_gt_u32_e64 %[m1], 16, %[t2]\n\t"
      "v_cmp_lt_u32_e64 %[m2], 31, %[t1]\n\t"
      "s_and_b64 %[m1], %[m1], %[m2]\n\t"
      "v_max_u32 %[t4], 16, %[t1]\n\t"
      "v_lshrrev_b32 %[t4], 4, %[t4]\n\t"
      "v_add_u32 %[t4], -1, %[t4]\n\t"
      "v_cndmask_b32_e64 %[t3], 0, %[b], %[m1]"
      : S16_OPERANDS, [sum] "+v"(sum)
      : [gbit] "v"(c.gbit), [rkey] "v"(c.rkey)
      : "vcc", "scc");
  len = (int)t4;
  last = t3;
}
#undef S16_LEVEL
#undef S16_TRIP
#undef S16_CAPTURE
#undef S16_SWEEP
#undef S16_OWN
#undef S16_MAX
#undef S16_SUM
#undef S16_OPERANDS

// component_fars() on sweep16_far.  The seed of a piece is the lowest cell of the first row of `remaining`: the row whose
// slice of the ballot has no bit below it.  What a sweep leaves of free_cells is the next `remaining`.
__device__ inline uint32_t component_fars16(const Grp<16> &g, const Sweep16Lane &c, uint32_t comps) {
  const uint32_t iso = comps & ~expand(g, comps);
  uint32_t remaining = comps & ~iso, fars = iso;
  while (true) {
    const uint64_t bal = __ballot(remaining != 0);
    if (bal == 0) break;
    const uint32_t slice = (uint32_t)(bal >> g.gbase);
    const uint32_t seed = (slice & c.below) == 0 ? (remaining & (0u - remaining)) : 0u;
    uint32_t free_cells = remaining ^ seed;
    fars |= sweep16_far(c, seed, free_cells);
    remaining = free_cells;
  }
  return fars;
}

// binary_stats_update() on sweep16: the statistics after editing the single cell `x`
__device__ inline void binary_stats_update16(const Grp<16> &g, uint32_t x, uint32_t p_old, uint32_t p_new, int &regions,
                                             int &path_len, uint32_t &fars, uint32_t &best PHASE_ARG, bool have_pre, uint32_t pre) {
  Sweep16Lane c;
  c.init(g);
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
  const uint32_t newfars = component_fars16(g, c, K);
  PHASE_MARK(4);  // first sweeps
  fars = (fars & ~touched) | newfars;
  int l;
  uint32_t b, count = (uint32_t)popc_m(fars);  // (summed over the group inside the sweep's wrap-up)
  sweep16_len(c, hit ? fars : newfars, p_new, l, b, count);
  PHASE_MARK(5);  // second sweep
  if (edited) {
    regions = (int)count;
    if (hit || l > path_len) {
      path_len = l;
      best = b;
    }
  }
}

// ---- the observe wave's encoder (development switches: A/B builds)
#ifndef PCGRL_STEP16_OBS_FIRST
#define PCGRL_STEP16_OBS_FIRST 1  // 0: encode_obs_any, the observe role as it was before encode_obs16
#endif
#ifndef PCGRL_STEP16_OBS_REGS
#define PCGRL_STEP16_OBS_REGS 1  // 0: encode_obs16, the encoder of §40 (conditional border trips, byte scatter in LDS)
#endif
// The largest launch that takes encode_obs16_regs.  Measured faster at 4 096 and 8 192 envs and slower at 16 384 and 65 536;
// nothing between 8 192 and 16 384 was measured, so the bound (that of the s_setprio below) is a guess inside that range.
constexpr int STEP16_OBS_REGS_MAX_ENVS = 8192;
#ifndef PCGRL_STEP16_OBS_PRIO
#define PCGRL_STEP16_OBS_PRIO 0  // 1: the observe wave at the simulate wave's issue priority up to its last observation store
#endif

// store_obs16 / store_obs16_nt with the chunk's distance from `dst` in the instruction's offset field (one address per lane
// for all chunks of a phase: a lane's chunks lie 256 bytes apart, twelve of them inside the field's 4 KB)
template <bool NT, int OFF>
__device__ __attribute__((always_inline)) inline void store_obs16_at(uint8_t *dst, const u32x4_t &w) {
  static_assert(OFF >= 0 && OFF < 4096, "the offset field of a global store");
  if constexpr (NT)
    asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc1 nt\n\ts_nop 1" : : "v"(dst), "v"(w), "n"(OFF) : "memory");
  else
    asm volatile("global_store_dwordx4 %0, %1, off offset:%2 " PCGRL_OBS_STORE_MODS "\n\ts_nop 1" : : "v"(dst), "v"(w), "n"(OFF) : "memory");
}

// Phase 1, chunk k = 16 * IT + row: stored when it lies in a border row, i.e. outside the 96 chunks from `lo` on
// (r = row - lo; one unsigned compare).  A trip whose mask is empty in the whole wave is skipped by the branch on exec.
template <bool NT, int IT>
__device__ __attribute__((always_inline)) inline void obs16_border_chunk(uint8_t *dst, int r, const u32x4_t *pat) {
  if ((unsigned)(r + 16 * IT) >= 96u) store_obs16_at<NT, 256 * IT>(dst, pat[IT % 3]);
}
template <bool NT>
__device__ __attribute__((always_inline)) inline void obs16_border(uint8_t *dst, int r, const u32x4_t *pat) {
  obs16_border_chunk<NT, 0>(dst, r, pat);
  obs16_border_chunk<NT, 1>(dst, r, pat);
  obs16_border_chunk<NT, 2>(dst, r, pat);
  obs16_border_chunk<NT, 3>(dst, r, pat);
  obs16_border_chunk<NT, 4>(dst, r, pat);
  obs16_border_chunk<NT, 5>(dst, r, pat);
  obs16_border_chunk<NT, 6>(dst, r, pat);
  obs16_border_chunk<NT, 7>(dst, r, pat);
  obs16_border_chunk<NT, 8>(dst, r, pat);
  obs16_border_chunk<NT, 9>(dst, r, pat);
  obs16_border_chunk<NT, 10>(dst, r, pat);
  obs16_border_chunk<NT, 11>(dst, r, pat);
}
template <bool NT>
__device__ __attribute__((always_inline)) inline void obs16_map_rows(uint8_t *dst, const uint4 *v) {
  store_obs16_at<NT, 0>(dst, u32x4_t{v[0].x, v[0].y, v[0].z, v[0].w});
  store_obs16_at<NT, 256>(dst, u32x4_t{v[1].x, v[1].y, v[1].z, v[1].w});
  store_obs16_at<NT, 512>(dst, u32x4_t{v[2].x, v[2].y, v[2].z, v[2].w});
  store_obs16_at<NT, 768>(dst, u32x4_t{v[3].x, v[3].y, v[3].z, v[3].w});
  store_obs16_at<NT, 1024>(dst, u32x4_t{v[4].x, v[4].y, v[4].z, v[4].w});
  store_obs16_at<NT, 1280>(dst, u32x4_t{v[5].x, v[5].y, v[5].z, v[5].w});
}

// encode_obs<PCGRL_PROB_BINARY, 16, /*FAST=*/true, uint32_t> (pcgrl_kernels2d.h) for this kernel: the same bytes -- the 32x32
// window around pos over the 16x16 map, one-hot with C = 3 channels, channel-last: 32 rows of six 16-byte chunks, chunk k of
// the env at byte 16 k -- in another order.  The map fills observation rows [16 - pos0, 32 - pos0): chunks [lo, lo + 96) with
// lo = 6 * (16 - pos0).  The other 96 chunks show nothing but "outside the map" (byte j of a row is 1 iff j % 3 == 0).
//
// Phase 1: the border chunks, from registers, before any LDS traffic.  Lane `row` owns chunks k = 16 it + row, it = 0..11;
// the pattern of chunk k starts at phase (16 k) % 3 = k % 3 = (it + row) % 3 of the dword sequence A B C A B C ..., so
// the lane keeps three dwords (the sequence from row % 3 on) as three quads and trip `it` stores quad it % 3.
// Phase 2: every lane builds the 96 bytes of its own map row in LDS as encode_obs does (the out-of-bounds pattern, then
// one byte pair per cell, the wave's four envs starting four cells apart: see there), and the group streams the 96
// map-row chunks: lane `row` takes the six k == row (mod 16) of [lo, lo + 96), i.e. t = d + 16 j with d = (row - lo) & 15 =
// (row + 6 pos0) & 15.  Chunk t of the map rows is chunk t % 6 of map row t / 6 and lies 16 (t + t / 6) bytes into the
// env's LDS rows (stride 112); with d = 6 m0 + q0, floor((q0 + 16 j) / 6) - floor(16 j / 6) is [q0 >= 2] for j = 1, 4,
// [q0 >= 4] for j = 2, 5 and 0 for j = 0, 3: three addresses per lane and six constant offsets, no division per chunk.
// (No row of LDS for the shared out-of-bounds row any more; the host still passes the same LDS size.)
__device__ inline void encode_obs16(const Grp<16> &g, const Params &p, int env, bool active, const uint32_t *b, const int *pos,
                                    uint8_t *lds) {
  constexpr int C = 3, FCH = 6, STRIDE = FCH * 16 + 16, ENV_BYTES = 32 * 32 * C;
  const bool nt = (p.obs16 & 2) != 0;  // (wave-uniform: scalar branches)
  uint8_t *base = p.obs + (size_t)env * ENV_BYTES;
  const int lo = 6 * (16 - pos[0]);
  if (active) {
    constexpr uint32_t SEQ0 = 0x01000001u, SEQ1 = 0x00010000u, SEQ2 = 0x00000100u;  // bytes 0-3, 4-7, 8-11 of the pattern
    const int r3 = g.row % 3;
    const uint32_t x0 = r3 == 0 ? SEQ0 : r3 == 1 ? SEQ1 : SEQ2;
    const uint32_t x1 = r3 == 0 ? SEQ1 : r3 == 1 ? SEQ2 : SEQ0;
    const uint32_t x2 = r3 == 0 ? SEQ2 : r3 == 1 ? SEQ0 : SEQ1;
    const u32x4_t pat[3] = {{x0, x1, x2, x0}, {x1, x2, x0, x1}, {x2, x0, x1, x2}};
    uint8_t *dst = base + g.row * 16;
    if (nt)
      obs16_border<true>(dst, g.row - lo, pat);
    else
      obs16_border<false>(dst, g.row - lo, pat);
  }
  uint8_t *row = lds + g.lane * STRIDE;
#pragma unroll
  for (int q = 0; q < FCH; q++) *(uint4 *)(row + q * 16) = oob_chunk<C>(q % C);
  const int left = pos[1] - 16;  // map column shown by obs column 0
  const int rot = PCGRL_OBS_ROT ? 4 * (g.lane >> 4) : 0;
#pragma unroll
  for (int x = 0; x < 16; x++) {
    const int xx = (x + rot) & 15;
    const int o = (xx - left) * C;  // always inside the window
    row[o] = 0;
    row[o + 1 + tile_at<1, uint32_t>(b, xx)] = 1;
  }
  if (active) {
    const int d = (g.row + 6 * pos[0]) & 15;
    const int m0 = (d >= 6 ? 1 : 0) + (d >= 12 ? 1 : 0), q0 = d - 6 * m0;
    const uint8_t *s0 = lds + g.gbase * STRIDE + 16 * (d + m0);
    const uint8_t *s1 = s0 + (q0 >= 2 ? 16 : 0), *s2 = s0 + (q0 >= 4 ? 16 : 0);
    const uint4 v[6] = {*(const uint4 *)s0,         *(const uint4 *)(s1 + 288),  *(const uint4 *)(s2 + 592),
                        *(const uint4 *)(s0 + 896), *(const uint4 *)(s1 + 1184), *(const uint4 *)(s2 + 1488)};
    uint8_t *dst = base + 16 * (lo + d);
    if (nt)
      obs16_map_rows<true>(dst, v);
    else
      obs16_map_rows<false>(dst, v);
  }
}

// ---- encode_obs16_regs (PCGRL_STEP16_OBS_REGS): the same bytes, chunks, phases and store flavours as
// encode_obs16 with fewer issue slots in front of the last observation store.  tools/step16_obs_regs.py restates both pieces.
//
// Addresses: one scalar base per wave (the observation of the wave's first env, `env0`) plus a 32-bit offset per lane and the
// instruction's signed offset field; no 64-bit adds.
//
// Piece A, the border chunks: they are the cyclic range [T, T + 96) mod 192 with T = lo + 96 = 192 - 6 pos0.  Lane `row` owns
// the chunks k = row (mod 16) as before, i.e. chunk 16 B + row of the 256-byte block B; with B0 = T >> 4 and r0 = T & 15 its
// border chunks lie in the five blocks B0 + 1 .. B0 + 5 (mod 12) and in ONE of the two boundary blocks: B0 when row >= r0,
// B0 + 6 otherwise.  Six unconditional stores per lane: store j >= 1 is block B0 + j for all sixteen lanes (256 contiguous,
// 256-byte-aligned bytes, as the conditional trips wrote them), store 0 the boundary chunk.  A block index wraps
// (B0 + j >= 12; B0 + 6 always does) by one compare on B0 and one select between two lane offsets 3072 bytes apart, the
// 256 j in the offset field (biased by -3072 so that neither offset is negative).  Chunk 16 B + row shows pattern phase
// (B + row) % 3 and 6 % 3 == 0, so the lane keeps the three quads rotated by (B0 + row) % 3 and store j takes quad j % 3.
// (A first form let lane `row` store its j-th border chunk counted from T, (lo + d + 96 + 16 j) mod 192: the same chunks per
// lane, but every store then straddles two blocks at a multiple of 96 bytes, and the launches of 16 384 and 65 536 envs lost
// 3 % to it: DESIGN §41.)
//
// Piece B, the map rows: lane `row` holds the 16 tile bits of its map row; cell c shows the bytes [0, !c, c], which sit at
// byte s = 48 - 3 pos1 of the 96-byte row, and s % 4 = pos1 % 4.  Four cells are three dwords, made from the cells' bits as
// bytes (one 24-bit multiply spreads four bits over four bytes: the four shifted copies do not overlap) and their
// complements with three v_perm_b32.  s is a multiple of 3, so the border pattern is a constant in map coordinates: the
// dword in front of the map's 48 bytes is 0x00000100 and the one behind them 0x01000001.  Thirteen v_alignbyte_b32 over
// [0x00000100, m0..m11, 0x01000001] with shift (4 - pos1 % 4) & 3 give the thirteen aligned dwords from dword (s - 1) >> 2
// of the row on, written over the prefilled row.  With pos1 % 4 == 0 the shift is 0 and the first of the thirteen is the
// border dword in FRONT of the map (dword s / 4 - 1 >= 2), which rewrites what the prefill put there; the last dword written
// is at most dword 23, so nothing reaches the row's 16-byte pad or the next lane's row.
// LDS banks (a write's bank is dword address % 32, conflicts count inside a 32-lane half): rows lie 28 dwords apart, so the
// 16 lanes of an env fall on 8 banks (2-way), and two envs at the same pos1 (always, with the narrow representation) on the
// same 8 (4-way): 13 dword writes x 4 = 52 array cycles per half, against 32 byte writes x 2 (2-way; the rotation kept the
// envs apart) = 64 before.  Derived from the addresses, not measured.
template <bool NT, int OFF>
__device__ __attribute__((always_inline)) inline void store_obs16_s(uint64_t sbase, uint32_t voff, const u32x4_t &w) {
  static_assert(OFF >= -4096 && OFF < 4096, "the offset field of a global store");
  if constexpr (NT)
    asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 sc1 nt\n\ts_nop 1" : : "v"(voff), "v"(w), "s"(sbase), "n"(OFF) : "memory");
  else
    asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 " PCGRL_OBS_STORE_MODS "\n\ts_nop 1"
                 :
                 : "v"(voff), "v"(w), "s"(sbase), "n"(OFF)
                 : "memory");
}
// store j >= 1 of piece A: `far` = the lane's offset in block B0 (+ 3072, the bias), `near` = the same twelve blocks lower
template <bool NT, int J>
__device__ __attribute__((always_inline)) inline void obs16_border_store(uint64_t sbase, uint32_t b0, uint32_t far, uint32_t near,
                                                                         const u32x4_t *pat) {
  store_obs16_s<NT, 256 * J - 3072>(sbase, b0 >= 12u - J ? near : far, pat[J % 3]);
}
template <bool NT>
__device__ __attribute__((always_inline)) inline void obs16_border_regs(uint64_t sbase, uint32_t b0, uint32_t first, uint32_t far,
                                                                        uint32_t near, const u32x4_t *pat) {
  store_obs16_s<NT, -3072>(sbase, first, pat[0]);
  obs16_border_store<NT, 1>(sbase, b0, far, near, pat);
  obs16_border_store<NT, 2>(sbase, b0, far, near, pat);
  obs16_border_store<NT, 3>(sbase, b0, far, near, pat);
  obs16_border_store<NT, 4>(sbase, b0, far, near, pat);
  obs16_border_store<NT, 5>(sbase, b0, far, near, pat);
}
template <bool NT>
__device__ __attribute__((always_inline)) inline void obs16_map_rows_regs(uint64_t sbase, uint32_t voff, const uint4 *v) {
  store_obs16_s<NT, 0>(sbase, voff, u32x4_t{v[0].x, v[0].y, v[0].z, v[0].w});
  store_obs16_s<NT, 256>(sbase, voff, u32x4_t{v[1].x, v[1].y, v[1].z, v[1].w});
  store_obs16_s<NT, 512>(sbase, voff, u32x4_t{v[2].x, v[2].y, v[2].z, v[2].w});
  store_obs16_s<NT, 768>(sbase, voff, u32x4_t{v[3].x, v[3].y, v[3].z, v[3].w});
  store_obs16_s<NT, 1024>(sbase, voff, u32x4_t{v[4].x, v[4].y, v[4].z, v[4].w});
  store_obs16_s<NT, 1280>(sbase, voff, u32x4_t{v[5].x, v[5].y, v[5].z, v[5].w});
}

// env0: the first env of the wave (wave-uniform); lane l belongs to env0 + l / 16
__device__ inline void encode_obs16_regs(const Grp<16> &g, const Params &p, int env0, bool active, const uint32_t *b, const int *pos,
                                         uint8_t *lds) {
  constexpr int C = 3, FCH = 6, STRIDE = FCH * 16 + 16, ENV_BYTES = 32 * 32 * C;
  const bool nt = (p.obs16 & 2) != 0;  // (wave-uniform: scalar branches)
  const uint64_t sbase = (uint64_t)(p.obs + (size_t)env0 * ENV_BYTES);
  // (24-bit multiplies throughout: the compiler takes v_mad_u64_u32, a quarter-rate instruction, for the plain products)
  const uint32_t d = (__umul24((uint32_t)pos[0], 6u) + (uint32_t)g.row) & 15u;
  const uint32_t c = __umul24((uint32_t)(16 - pos[0]), 6u) + d;                     // lo + d: the lane's first map-row chunk
  const uint32_t voff = __umul24((uint32_t)(g.lane >> 4), ENV_BYTES) + 16u * c;  // ... and its distance from sbase
  if (active) {
    const uint32_t T = 192u - __umul24((uint32_t)pos[0], 6u), b0 = T >> 4, r0 = T & 15u;
    const uint32_t x = b0 + (uint32_t)g.row;                             // < 32, where x / 3 == (11 x) >> 5
    const uint32_t ph = x - 3u * (__umul24(x, 11u) >> 5);                // (B0 + row) % 3
    // dword `ph`, ph + 1, ph + 2 of the pattern sequence 0x01000001, 0x00010000, 0x00000100, ...: the pattern's bytes from
    // byte ph, ph + 1 and 2 + ph on
    const uint32_t x0 = __builtin_amdgcn_alignbyte(0x00010000u, 0x01000001u, ph);
    const uint32_t x1 = __builtin_amdgcn_alignbyte(0x00010000u, 0x01000001u, ph + 1u);
    const uint32_t x2 = __builtin_amdgcn_alignbyte(0x01000001u, 0x00000100u, ph);
    const u32x4_t pat[3] = {{x0, x1, x2, x0}, {x1, x2, x0, x1}, {x2, x0, x1, x2}};
    const uint32_t near = __umul24((uint32_t)(g.lane >> 4), ENV_BYTES) + 256u * b0 + 16u * (uint32_t)g.row;
    const uint32_t far = near + (uint32_t)ENV_BYTES;
    const uint32_t first = (uint32_t)g.row < r0 ? near + 6u * 256u : b0 >= 12u ? near : far;  // block B0 + 6 - 12, or B0
    if (nt)
      obs16_border_regs<true>(sbase, b0, first, far, near, pat);
    else
      obs16_border_regs<false>(sbase, b0, first, far, near, pat);
  }
  uint8_t *row = lds + g.lane * STRIDE;
#pragma unroll
  for (int q = 0; q < FCH; q++) *(uint4 *)(row + q * 16) = oob_chunk<C>(q % C);
  uint32_t m[14];
  m[0] = 0x00000100u;
  m[13] = 0x01000001u;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint32_t spread = __umul24((b[0] >> (4 * q)) & 15u, 0x204081u);  // bit i of the four at bit 8 i (and junk elsewhere)
    const uint32_t solid = spread & 0x01010101u, empty = solid ^ 0x01010101u;
    m[3 * q + 1] = __builtin_amdgcn_perm(empty, solid, 0x0c00040cu);  // [0, !c0, c0, 0]
    m[3 * q + 2] = __builtin_amdgcn_perm(empty, solid, 0x060c0105u);  // [!c1, c1, 0, !c2]
    m[3 * q + 3] = __builtin_amdgcn_perm(empty, solid, 0x03070c02u);  // [c2, 0, !c3, c3]
  }
  const uint32_t sh = (uint32_t)(-pos[1]) & 3u;
  uint32_t *w = (uint32_t *)row + ((__mul24(pos[1], -3) + 47) >> 2);
#pragma unroll
  for (int i = 0; i < 13; i++) w[i] = __builtin_amdgcn_alignbyte(m[i + 1], m[i], sh);
  if (active) {
    const uint32_t m0 = (d >= 6u ? 1u : 0u) + (d >= 12u ? 1u : 0u), q0 = d - 6u * m0;
    const uint8_t *s0 = lds + g.gbase * STRIDE + 16 * (d + m0);
    const uint8_t *s1 = s0 + (q0 >= 2u ? 16 : 0), *s2 = s0 + (q0 >= 4u ? 16 : 0);
    const uint4 v[6] = {*(const uint4 *)s0,         *(const uint4 *)(s1 + 288),  *(const uint4 *)(s2 + 592),
                        *(const uint4 *)(s0 + 896), *(const uint4 *)(s1 + 1184), *(const uint4 *)(s2 + 1488)};
    if (nt)
      obs16_map_rows_regs<true>(sbase, voff, v);
    else
      obs16_map_rows_regs<false>(sbase, voff, v);
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
#if PCGRL_STEP16_OBS_PRIO
    if (p.n_envs <= 8192) __builtin_amdgcn_s_setprio(3);  // (where the simulate wave raises its own, below)
#endif
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
#if PCGRL_STEP16_OBS_FIRST && PCGRL_STEP16_OBS_REGS
    // (the register encoder where a SIMD holds few waves and the launch waits for the observe waves' issue slots; from
    // 16 384 envs on the launch is bound by its writes and measured 1 - 2 % faster with encode_obs16: DESIGN §41)
    if (p.n_envs <= STEP16_OBS_REGS_MAX_ENVS)
      encode_obs16_regs(g, p, (int)((blockIdx.x * STEP16_PAIRS + pair) * EPW), active, b, pos, lds);
    else
      encode_obs16(g, p, e, active, b, pos, lds);
#elif PCGRL_STEP16_OBS_FIRST
    encode_obs16(g, p, e, active, b, pos, lds);
#else
    encode_obs_any<PROB, LPE, true, M>(g, p, e, active, b, pos, lds);
#endif
#if PCGRL_STEP16_OBS_PRIO
    if (p.n_envs <= 8192) __builtin_amdgcn_s_setprio(0);  // (the flood yields to the simulate waves again)
#endif
    [[maybe_unused]] const unsigned long long _tr_issued = TRACE_NOW();  // (behind the last observation store, before the flood)
    // PREFLOOD: the component of the next edit's cell, flooded ahead of time for the next launch's simulate wave
    const M xbit = (active && g.row == pos[0]) ? (M(1) << pos[1]) : M(0);
    const M comp = flood(g, xbit, (~b[0] & colmask) | xbit);
    if (active) pl[16 * PRE_PLANE] = comp | (M)PRE_VALID;
    TRACE_PUT(2, _tr0);
    TRACE_PUT(3, _tr_issued);
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
