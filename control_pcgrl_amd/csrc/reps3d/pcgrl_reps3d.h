// reps3d/pcgrl_reps3d.h -- gfx950 kernels for minecraft_3D_maze under the turtle and wide representations.
//
// Reference (paths relative to control_pcgrl/): envs/reps/turtle_rep.py:31-44 reset, :84-107 update_pos;
// envs/reps/wide_rep.py update; envs/pcgrl_env.py:267-342 step; envs/pcgrl_env_3D.py; the problem side is
// ../pcgrl_kernels3d.h (move table, slot cache, FIFO searches, region count, overlay), used here as it is: everything below
// is what depends on the representation.
//
//   turtle  Discrete(4 + n_tiles).  Actions 0..3 move the position along the FIRST TWO array axes only (turtle_rep._dirs holds
//           2-tuples and update_pos walks enumerate(_dirs[action])), clamped at the edges; the third coordinate keeps the
//           value drawn at reset for the whole episode.  Actions 4, 5 write tile action - 4 at the position.  reset draws
//           the position -- three doubles of the representation's generator -- BEFORE the map.  A move is a step with
//           change == 0: no statistics, reward 0, the window moves.
//   wide    one int32 per env = the C-order flat index over (d0, d1, d2, n_tiles); the reference indexes the map with
//           action[:-1] directly (there is no ActionMap in this stack, so nothing is transposed).  The observation is the
//           whole map, [d0][d1][d2][3] one-hot (AIR, DIRT, path overlay), no out-of-bounds channel and no crop.
//
// The step kernels keep the wave roles of m3_kernel (simulate, observe, helper).  The observe wave replays the action on its
// own copy of the tile bits: turtle computes the post-step position from the action (one load, a clamp), wide takes the
// edited cell from it, so neither waits for the simulate wave; the overlay shown is that of the previous statistics update.
// A wide row is 3 * n_cells bytes (1029 at 7^3), so rows start at any byte: the encoder stores whole 16-byte words between
// the first and the last 16-byte boundary of the row and at most 15 single bytes on either side of them.
#pragma once
#include <hip/hip_runtime.h>

#include "../pcgrl_dispatch.h"
#include "../pcgrl_kernels3d.h"

namespace pcgrl {

hipError_t launch_3d_turtle(KernelId id, const Params &p, int cpl, hipStream_t s);
hipError_t launch_3d_wide(KernelId id, const Params &p, int cpl, hipStream_t s);

#ifdef PCGRL_KERNEL_TU

// What an action does before anything is computed: the (clamped) move or the cell it writes.  pos = (z, y, x) = array
// indices (0, 1, 2).  `cell` < 0: nothing is written (a move, or a bad action).
template <int REP>
__device__ inline void r3_decode(const M3Ctx &c, int action, int *pos, int &n_step, bool &bad, int &cell, int &tile) {
  cell = -1;
  tile = 0;
  if constexpr (REP == PCGRL_REP_TURTLE) {
    bad = action < 0 || action >= 6;
    if (bad) return;
    if (action < 4) {  // _dirs = [(-1,0), (1,0), (0,-1), (0,1)] on axes 0 and 1; _wrap is False
      const int d = (action & 1) ? 1 : -1;
      if (action < 2)
        pos[0] = min(max(pos[0] + d, 0), c.Z - 1);
      else
        pos[1] = min(max(pos[1] + d, 0), c.Y - 1);
    } else {
      tile = action - 4;
      cell = (pos[0] * c.Y + pos[1]) * c.X + pos[2];
    }
  } else {
    bad = action < 0 || action >= 2 * c.n_cells;
    if (bad) return;
    cell = action >> 1;
    tile = action & 1;
    pos[0] = cell / c.YX;
    const int q = cell - pos[0] * c.YX;
    pos[1] = q / c.X;
    pos[2] = q - pos[1] * c.X;
  }
  n_step++;
}

// the turtle's start position: three draws of the representation's generator, before the map (turtle_rep.py:31-44)
template <int REP>
__device__ inline void r3_reset_pos(const M3Ctx &c, Pcg &rr, int *pos) {
  pos[0] = pos[1] = pos[2] = 0;
  if constexpr (REP == PCGRL_REP_TURTLE) {
    pos[0] = (int)(rr.next_double() * (double)c.Z);
    pos[1] = (int)(rr.next_double() * (double)c.Y);
    pos[2] = (int)(rr.next_double() * (double)c.X);
  }
}

// wide observation: byte b of the env's row = (code(cell b / 3) == b % 3), code = 2 on the overlay, else the tile.
// `part` of `nparts`: the share of one of several observe waves.
__device__ inline void r3_encode_wide(const uint32_t *dirt, const uint32_t *over, const M3Ctx &c, const Params &p, int env,
                                      bool show_path, uint8_t *obs_base, int part = 0, int nparts = 1) {
  if (obs_base == nullptr) return;
  const int RB = 3 * c.n_cells;
  uint8_t *row = obs_base + (size_t)env * (size_t)RB;
  const int head = min(RB, (int)((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u));  // bytes in front of the first 16-byte boundary
  const int nchunk = (RB - head) >> 4;
  const int tail0 = head + 16 * nchunk;
  // 7 consecutive cells from cell c0 on: bit i of .x / .y = low / high bit of the code of cell c0 + i
  auto codes_from = [&](int c0) -> uint2 {
    const int w = c0 >> 5, s = c0 & 31;
    const uint32_t db = (uint32_t)((((uint64_t)dirt[w] | ((uint64_t)dirt[w + 1] << 32)) >> s));
    const uint32_t ob = show_path ? (uint32_t)((((uint64_t)over[w] | ((uint64_t)over[w + 1] << 32)) >> s)) : 0u;
    return make_uint2(db & ~ob, ob);
  };
  auto byte_at = [&](int b) -> uint32_t {
    const int c0 = (int)((uint32_t)b / 3u), ch = b - 3 * c0;
    const uint2 m = codes_from(c0);
    return (uint32_t)((int)((m.x & 1u) | ((m.y & 1u) << 1)) == ch);
  };
  auto chunk = [&](int r0) -> uint4 {  // the 16 bytes from row offset r0
    const int c0 = (int)((uint32_t)r0 / 3u), ph = r0 - 3 * c0;
    const uint2 m = codes_from(c0);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int kk = ph + j, co = (kk * 11) >> 5, ch = kk - 3 * co;  // co = kk / 3 for kk <= 17
      const int code = (int)(((m.x >> co) & 1u) | (((m.y >> co) & 1u) << 1));
      w[j >> 2] |= (uint32_t)(code == ch) << (8 * (j & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
  };
  if (part == 0 && c.lane < head) row[c.lane] = (uint8_t)byte_at(c.lane);
  if (part == nparts - 1 && c.lane < RB - tail0) row[tail0 + c.lane] = (uint8_t)byte_at(tail0 + c.lane);
  const int ch_lo = (int)((long long)nchunk * part / nparts), ch_hi = (int)((long long)nchunk * (part + 1) / nparts);
  uint4 *dst = (uint4 *)(row + head);
  const bool nt = (p.obs16 & 2) != 0;
  int ch = ch_lo + c.lane;
  for (; ch + 64 < ch_hi; ch += 128) {  // two chunks per trip: the store is an asm statement the next chunk's LDS reads do not pass
    const uint4 v0 = chunk(head + 16 * ch), v1 = chunk(head + 16 * (ch + 64));
    if (nt) {
      store_obs16_nt(dst + ch, v0);
      store_obs16_nt(dst + ch + 64, v1);
    } else {
      store_obs16(dst + ch, v0);
      store_obs16(dst + ch + 64, v1);
    }
  }
  for (; ch < ch_hi; ch += 64) store_obs16(dst + ch, chunk(head + 16 * ch));
}

// the observation of either representation.  WIN as in m3_encode_obs (turtle); scratch: the row masks of that encoder
template <int REP, int WIN>
__device__ inline void r3_encode(const uint32_t *dirt, const uint32_t *over, const M3Ctx &c, const Params &p, int env, const int *pos,
                                 bool show_path, uint2 *scratch, int scratch_rows, uint8_t *obs_base, int part = 0, int nparts = 1) {
  if constexpr (REP == PCGRL_REP_WIDE)
    r3_encode_wide(dirt, over, c, p, env, show_path, obs_base, part, nparts);
  else
    m3_encode_obs<WIN>(dirt, over, c, p, env, pos, show_path, scratch, scratch_rows, obs_base, part, nparts);
}

// MODE: M3_STEP, M3_RESET, M3_OBSERVE, M3_ROLLOUT (get_state, stats_for_grids and last_episode do not depend on the
// representation: the engine launches m3_kernel's).  SC, DIM, the waves of a step workgroup and the write-back rules are
// those of m3_kernel.
template <int MODE, int SC, int REP, int DIM = 0>
__global__ __launch_bounds__(MODE == M3_STEP ? 64 * (2 + m3_observers<SC>()) : 64, (MODE == M3_STEP && SC == 0) ? 4 : 1)
void r3_kernel(Params p, int cpl) {
  constexpr int PW = M3C<SC>::PW;
  constexpr bool HELP = MODE == M3_STEP, HELP_S = HELP && SC == 0;
  constexpr int WIN = REP == PCGRL_REP_WIDE ? 0 : 2 * DIM;
  if (MODE == M3_STEP) touch_kernarg(p);
  __shared__ M3Env<SC> E;
  __shared__ M3Work<SC> W;
  __shared__ M3Mail mail;
  M3Work<SC> *WH = nullptr;  // the helper wave's workspace
  if constexpr (HELP_S) {
    __shared__ M3Work<SC> wh_;
    WH = &wh_;
  }
  __shared__ M3ObsLds<SC> O;
  M3Ctx c;
  c.lane = (int)__lane_id();
  c.Z = DIM ? DIM : p.cfg.dims[0];
  c.Y = DIM ? DIM : p.cfg.dims[1];
  c.X = DIM ? DIM : p.cfg.dims[2];
  if (DIM) cpl = (DIM * DIM * DIM + 63) / 64;
  c.YX = c.Y * c.X;
  c.n_cells = c.Z * c.YX;
#ifdef PCGRL_PHASE_TIMING
  c.knob = 0;
#endif
  c.L = m3_layout(c.Z, c.Y, c.X);
  c.dirt = E.rec;
  c.over = E.rec + c.L.o_over;
  c.col = (uint16_t *)(E.rec + c.L.o_col);
  c.slots = E.rec + c.L.o_slots;
  c.mv = (int16_t *)(E.rec + c.L.o_mv);
  const int nw = c.L.nw, n_slots = c.L.n_slots;
  const int env = blockIdx.x;
  constexpr int NS = M3_NS;
  PHASE_DECL();
  uint32_t *grec = (uint32_t *)p.planes + (size_t)env * c.L.rec_words;
  EnvState *S = &p.st[env];

  if constexpr (HELP) {
    if (threadIdx.x == 0) {
      mail.seq = 0;
      mail.done = 0;
      mail.rseq = 0;
      mail.rdone = 0;
      mail.cancel = 0;
      mail.exit = 0;
      mail.obs_read = 0;
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 1 + m3_observers<SC>()) {
      m3_helper<SC, HELP_S>(p, HELP_S ? *WH : W, c, mail PHASE_PASS);
      return;
    }
  }
  if constexpr (MODE == M3_STEP) {
    // ------------------------------------------------------------------------------------------ observe wave
    constexpr int NOBS = m3_observers<SC>();
    const int wave_id = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave_id >= 1 && wave_id <= NOBS) {
      if (p.obs == nullptr) return;  // (the simulate wave skips the wait in that case, too)
      const int part = wave_id - 1;
      uint32_t *obits = O.bits[part];
      for (int i = c.lane; i < 2 * nw; i += 64) obits[i] = grec[i];
      int pos[3] = {S->pos[0], S->pos[1], S->pos[2]};
      int n_step = S->n_step, iteration = S->iteration, changes = S->changes;
      const int action = p.actions[env];
      const bool upd_only = p.update_only != 0;
      Pcg rp, rr;
      rp.load(p.rng[env].prob);
      rr.load(p.rng[env].rep);
      // the simulate wave overwrites the env's state only after every observe wave holds its copy of the old one
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (c.lane == 0) __hip_atomic_fetch_add(&mail.obs_read, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      uint32_t *odirt = obits, *oover = obits + nw;
      iteration += upd_only ? 0 : 1;
      bool bad = false, change = false;
      int cell = -1, tile = 0;
      r3_decode<REP>(c, action, pos, n_step, bad, cell, tile);  // the post-step position comes from the action alone
      if (cell >= 0) {
        change = m3_bit(odirt, cell) != (tile != 0);
        if (change && c.lane == 0) odirt[cell >> 5] ^= 1u << (cell & 31);
      }
      changes += (change && !upd_only) ? 1 : 0;
      bool done = !upd_only && iteration > p.cfg.max_iterations;
      if (p.cfg.max_changes >= 0) done = done || (!upd_only && changes > p.cfg.max_changes);
      bool show = true;
      if (done && p.auto_reset != 0) {  // first observation of the new episode: no overlay (PcgrlEnv.reset)
        r3_reset_pos<REP>(c, rr, pos);
        m3_reset_rng(odirt, c, p, cpl, rp, rr);
        show = false;
      }
      r3_encode<REP, WIN>(odirt, oover, c, p, env, pos, show, O.rows, (int)(sizeof(O.rows) / sizeof(uint2)), p.obs, part, NOBS);
      return;
    }
    __builtin_amdgcn_s_setprio(3);  // the simulate wave's dependent chain issues ahead of the observe wave on its SIMD
  }

  if constexpr (MODE == M3_OBSERVE) {
    // reset()/observe(): no path overlay (PcgrlEnv.reset does not call process_observation)
    for (int i = c.lane; i < 2 * nw; i += 64) E.rec[i] = grec[i];
    const int pos[3] = {S->pos[0], S->pos[1], S->pos[2]};
    r3_encode<REP, 0>(c.dirt, c.over, c, p, env, pos, false, (uint2 *)W.info, M3C<SC>::CELLS / 2, p.obs);
    return;
  }

  // search tables of this wave
  uint32_t epoch = 0, trip = 0;
  uint32_t dirty_hdr = 0, dirty_full = 0;  // slots whose header / whose whole record differs from the copy in HBM
  auto init_work = [&]() {
    for (int i = c.lane; i < c.n_cells; i += 64) W.best[i] = make_uint2(0u, 0xFFFFFFFFu);
  };
  PM<PW> notx0, notxl;
  m3_edge_masks<PW>(p, notx0, notxl);
  auto plane_of = [&](const uint32_t *dirt) { return c.lane < c.Z ? m3_plane_air<PW>(dirt, c, c.lane) : pm_zero<PW>(); };
  // statistics of a map the kernel has not seen before: columns, move table, no cached slots
  auto fresh_stats = [&](int32_t *st, bool &ovf) {
    const PM<PW> air = plane_of(c.dirt);
    for (int i = c.lane; i < c.L.o_slots - c.L.o_col; i += 64) E.rec[c.L.o_col + i] = 0;
    m3_build_cols<PW>(c, air);
    m3_build_moves(c);
    if (c.lane < n_slots) *(uint4 *)c.hdr(c.lane) = make_uint4(0u, 0u, 0u, 0u);
    dirty_hdr = (1u << n_slots) - 1u;
    st[0] = m3_regions<PW>(c, air, notx0, notxl);
    m3_paths<SC>(E, W, c, air, st, epoch, trip, dirty_full, ovf, nullptr, nullptr PHASE_PASS);
  };
  auto store_record = [&]() {
    for (int i = c.lane; i < c.L.rec_words / 4; i += 64) ((uint4 *)grec)[i] = ((const uint4 *)E.rec)[i];
  };

  int32_t st[NS];
  bool ovf = false;
  EnvTargets<NS> trg;
  Pcg rp, rr;

  if constexpr (MODE == M3_RESET) {
    if (p.mask != nullptr && p.mask[env] == 0) return;
    for (int i = c.lane; i < 2 * nw; i += 64) E.rec[i] = grec[i];
    init_work();
    trg.load(p, env, false);
    if (p.refresh_only) {  // statistics (and the path overlay) of the current map, nothing else
      fresh_stats(st, ovf);
      if (ovf && c.lane == 0) atomicOr(p.err, 4);
      store_record();
      if (c.lane == 0) {
        S->last_loss = trg.loss(p.cfg, st);
        S->flags = 0;
        for (int k = 0; k < NS; k++) {
          S->stats[k] = st[k];
          if (p.stats_out) p.stats_out[(size_t)env * NS + k] = st[k];
        }
      }
      return;
    }
    int pos[3] = {0, 0, 0};
    if (p.init_grids) {
      m3_load_bytes(c.dirt, c, p.init_grids + (size_t)env * c.n_cells);
      if (p.init_pos && REP == PCGRL_REP_TURTLE) {  // (clamped: a position is an index into the map)
        pos[0] = min(max(p.init_pos[(size_t)env * 3 + 0], 0), c.Z - 1);
        pos[1] = min(max(p.init_pos[(size_t)env * 3 + 1], 0), c.Y - 1);
        pos[2] = min(max(p.init_pos[(size_t)env * 3 + 2], 0), c.X - 1);
      }
    } else {
      rp.load(p.rng[env].prob);
      rr.load(p.rng[env].rep);
      r3_reset_pos<REP>(c, rr, pos);
      m3_reset_rng(c.dirt, c, p, cpl, rp, rr);
      if (c.lane == 0) {
        rr.store(p.rng[env].rep);
        rp.store(p.rng[env].prob);
      }
    }
    fresh_stats(st, ovf);
    int n_step = 0, iteration = 0, changes = 0;
    double ep_return = 0.0;
    if (p.set_state) {  // pcgrl_set_state: injected map, the caller's counters / return
      if (p.in_counters) {
        iteration = p.in_counters[(size_t)env * 4 + 0];
        changes = p.in_counters[(size_t)env * 4 + 1];
        n_step = p.in_counters[(size_t)env * 4 + 2];
      }
      if (p.in_ep_return) ep_return = p.in_ep_return[env];
    }
    trg.load(p, env, true);
    const double last_loss = trg.loss(p.cfg, st);
    if (ovf && c.lane == 0) atomicOr(p.err, 4);
    store_record();
    if (c.lane == 0) {
      trg.write_ctrl_obs(p, env, st);
      trg.commit(p, env);
      S->pos[0] = pos[0];
      S->pos[1] = pos[1];
      S->pos[2] = pos[2];
      S->n_step = n_step;
      S->iteration = iteration;
      S->changes = changes;
      S->flags = 0;
      S->last_loss = last_loss;
      S->ep_return = ep_return;
      for (int k = 0; k < NS; k++) S->stats[k] = st[k];
    }
    return;
  }

  if constexpr (MODE == M3_STEP || MODE == M3_ROLLOUT) {
    // ---- everything of the old state is requested before anything is waited for
    constexpr int CH = SC == 0 ? (M3C<0>::REC / 4 + 63) / 64 : 1;
    uint4 rch[CH];
    if (SC == 0) {
#pragma unroll
      for (int k = 0; k < CH; k++) {
        const int i = c.lane + 64 * k;
        rch[k] = i < c.L.rec_words / 4 ? ((const uint4 *)grec)[i] : make_uint4(0u, 0u, 0u, 0u);
      }
    }
    int pos[3] = {S->pos[0], S->pos[1], S->pos[2]};
    int n_step = S->n_step, iteration = S->iteration, changes = S->changes, flags = S->flags;
    double last_loss = S->last_loss, ep_return = S->ep_return;
    for (int k = 0; k < NS; k++) st[k] = S->stats[k];
    int action0 = p.actions[env];
    trg.load(p, env, false);
    init_work();
    if (SC == 0) {
#pragma unroll
      for (int k = 0; k < CH; k++) {
        const int i = c.lane + 64 * k;
        if (i < c.L.rec_words / 4) ((uint4 *)E.rec)[i] = rch[k];
      }
    } else {
      // size class 1: the move table and the cached start planes follow only for a step that changes the map or resets
      const int s0 = (c.L.o_slots & ~3) / 4, s1 = c.L.rec_words / 4;
      m3_copy_batched<4>((uint4 *)E.rec, (const uint4 *)grec, 0, s0, c.lane);
      bool need_rest = true;
      if constexpr (MODE == M3_STEP) {
        int pos0[3] = {pos[0], pos[1], pos[2]}, ns0 = 0, cell0 = -1, tile0 = 0;
        bool bad0 = false;
        r3_decode<REP>(c, action0, pos0, ns0, bad0, cell0, tile0);
        const bool ch0 = cell0 >= 0 && m3_bit(c.dirt, cell0) != (tile0 != 0);
        const bool reset0 = p.auto_reset != 0 && p.update_only == 0 &&
                            (iteration + 1 > p.cfg.max_iterations || (p.cfg.max_changes >= 0 && changes + (ch0 ? 1 : 0) > p.cfg.max_changes));
        need_rest = ch0 || reset0;
      }
      if (need_rest) m3_copy_batched<16>((uint4 *)E.rec, (const uint4 *)grec, s0, s1, c.lane);
    }
    const int K = MODE == M3_ROLLOUT ? p.n_steps : 1;
    const size_t N = (size_t)p.n_envs;
    bool any_reset = false, whole_record = false, edited = false, mv_chg = false, upd_exit = false, over_dirty = false;
    bool ovf_any = false;
    int mv_cell = 0, col_word = 0;
    for (int k = 0; k < K; k++) {
      const size_t o = (size_t)k * N + (size_t)env;  // index of this step's outputs
      uint8_t *obs_k = p.obs == nullptr ? nullptr
                       : (MODE == M3_ROLLOUT && !p.obs_last_only ? p.obs + (size_t)k * N * (size_t)p.obs_env_bytes : p.obs);
      const bool want_obs = MODE == M3_ROLLOUT && obs_k != nullptr && (!p.obs_last_only || k == K - 1);  // (M3_STEP: the observe wave)
      // ---- step (envs/pcgrl_env.py:267-342)
      const int action = k == 0 ? action0 : p.actions[o];
      const bool upd_only = p.update_only != 0;
      iteration += upd_only ? 0 : 1;
      bool bad = false, change = false;
      int cell = -1, tile = 0;
      r3_decode<REP>(c, action, pos, n_step, bad, cell, tile);
      int ex = 0, ey = 0, ez = 0;
      if (cell >= 0) {
        ez = cell / c.YX;
        const int q = cell - ez * c.YX;
        ey = q / c.X;
        ex = q - ey * c.X;
        change = m3_bit(c.dirt, cell) != (tile != 0);
        if (change) {
          if (c.lane == 0) {
            atomicXor(&c.dirt[cell >> 5], 1u << (cell & 31));
            atomicXor((uint32_t *)c.col + (q >> 1), (1u << ez) << (16 * (q & 1)));
          }
          col_word = q >> 1;
          if (edited) whole_record = true;  // (rollout: more than one edit per launch)
          edited = true;
          dirty_hdr |= m3_update_moves(c, ex, ey, ez, mv_chg, mv_cell);
        }
      } else if (bad && c.lane == 0) {
        atomicOr(p.err, 1);
      }
      if (upd_only) {  // rep.update() only: map, position (the observe wave shows the stale overlay)
        if (change) flags |= ENV_STATS_DIRTY;
        upd_exit = true;
        break;
      }
      changes += change ? 1 : 0;
      bool done = iteration > p.cfg.max_iterations;
      if (p.cfg.max_changes >= 0) done = done || changes > p.cfg.max_changes;
      const bool do_reset = done && p.auto_reset != 0;
      // the observation is assembled BEFORE the stats refresh (pcgrl_env.py:298-299 vs :314-323)
      if (!do_reset && want_obs) r3_encode<REP, WIN>(c.dirt, c.over, c, p, env, pos, true, (uint2 *)W.info, M3C<SC>::CELLS / 2, obs_k);
      if (change) {
        const PM<PW> air = plane_of(c.dirt);
        const int32_t st_old[NS] = {st[0], st[1], st[2]};
        int rjob = 0;
        if constexpr (HELP) {  // the helper wave counts the regions while this wave searches
          if (c.lane == 0) {
            rjob = m3_ld(&mail.rseq) + 1;
            mail.r_eq = ey * c.X + ex;
            mail.r_ez = ez;
            mail.r_kind = (flags & ENV_STATS_DIRTY) ? 2 : (tile == 0 ? 0 : 1);
            mail.r_old = st[0];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            m3_st(&mail.rseq, rjob);
          }
          rjob = __builtin_amdgcn_readfirstlane(rjob);
        } else if (flags & ENV_STATS_DIRTY) {  // after pcgrl_update: from scratch, like the reference's get_stats
          st[0] = m3_regions<PW>(c, air, notx0, notxl);
        } else {
          PM<PW> A = air;  // the planes without the edited cell
          if (c.lane == ez) {
            PM<PW> e = pm_zero<PW>();
            pm_set(e, ey * c.X + ex);
            A = A & ~e;
          }
          st[0] = m3_regions_update<PW>(c, A, notx0, notxl, ey * c.X + ex, ez, tile == 0, st[0]);
        }
        flags &= ~ENV_STATS_DIRTY;
        m3_paths<SC>(E, W, c, air, st, epoch, trip, dirty_full, ovf, WH, HELP_S ? &mail : nullptr PHASE_PASS);
        over_dirty = true;
        if constexpr (HELP) {
          while (__builtin_amdgcn_readfirstlane(m3_ld(&mail.rdone)) != rjob) __builtin_amdgcn_s_sleep(1);
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          st[0] = __builtin_amdgcn_readfirstlane(m3_ld(&mail.r_out));
        }
        if (ovf)  // queue overflow: reported (pcgrl_poll_error), no statistics of an unfinished search are handed out
          for (int i = 0; i < NS; i++) st[i] = st_old[i];
      }
      if (ovf) {  // as in m3_kernel: every cached start plane is dropped and the env is marked stale
        if (c.lane < n_slots) *(uint4 *)c.hdr(c.lane) = make_uint4(0u, 0u, 0u, 0u);
        dirty_hdr = (1u << n_slots) - 1u;
        flags |= ENV_STATS_DIRTY;
        ovf_any = true;
        ovf = false;
      }
      const double loss = trg.loss(p.cfg, st);
      const double rew = loss - last_loss;
      last_loss = loss;
      ep_return += rew;
      if (c.lane == 0) {
        if (p.reward) p.reward[o] = (float)rew;
        if (p.reward64) p.reward64[o] = rew;
        if (p.done) p.done[o] = done ? 1 : 0;
        if (p.stats_out)
          for (int i = 0; i < NS; i++) p.stats_out[o * NS + i] = st[i];
      }
      if (do_reset) {
        if (!any_reset) {
          rp.load(p.rng[env].prob);  // (only this wave writes them, at the end)
          rr.load(p.rng[env].rep);
        }
        if (c.lane == 0) {
          latch_episode<NS>(p, env, S, ep_return, iteration, st);
          accumulate_episode<NS>(S);
        }
        r3_reset_pos<REP>(c, rr, pos);
        m3_reset_rng(c.dirt, c, p, cpl, rp, rr);
        any_reset = true;
        whole_record = true;
        fresh_stats(st, ovf);
        flags = 0;
        n_step = iteration = changes = 0;
        ep_return = 0.0;
        trg.load(p, env, true);
        last_loss = trg.loss(p.cfg, st);
        if (c.lane == 0) trg.commit(p, env);
        if (want_obs) r3_encode<REP, WIN>(c.dirt, c.over, c, p, env, pos, false, (uint2 *)W.info, M3C<SC>::CELLS / 2, obs_k);
      }
    }
    if ((ovf || ovf_any) && c.lane == 0) atomicOr(p.err, 4);
    // ---- write back, once the observe waves have read the old state
    if (HELP && c.lane == 0) m3_st(&mail.exit, 1);
    if (MODE == M3_STEP && p.obs != nullptr) {
      while (__builtin_amdgcn_readfirstlane(m3_ld(&mail.obs_read)) != m3_observers<SC>()) __builtin_amdgcn_s_sleep(1);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    if (whole_record) {
      store_record();
    } else if (SC == 0) {
      // size class 0: every piece fits one pass of the wave: all LDS reads are issued before the first store
      constexpr int NSL = M3C<0>::SLOTS;
      const int l_nw = c.lane < nw ? c.lane : 0;
      const uint32_t v_dirt = c.dirt[l_nw], v_over = c.over[l_nw], v_col = E.rec[c.L.o_col + col_word];
      const uint2 v_mv = ((const uint2 *)(E.rec + c.L.o_mv))[mv_chg ? mv_cell : 0];
      const uint32_t dm = dirty_hdr | dirty_full;
      uint32_t v_slot[NSL];
#pragma unroll
      for (int s = 0; s < NSL; s++) {
        const int n = ((dirty_full >> s) & 1u) ? c.L.slot_words : M3_SLOT_HDR;
        v_slot[s] = (s < n_slots && ((dm >> s) & 1u) && c.lane < n) ? E.rec[c.L.o_slots + s * c.L.slot_words + c.lane] : 0u;
      }
      if (edited) {
        if (c.lane < nw) grec[c.lane] = v_dirt;
        if (c.lane == 0) grec[c.L.o_col + col_word] = v_col;
        if (mv_chg) ((uint2 *)(grec + c.L.o_mv))[mv_cell] = v_mv;
      }
      if (over_dirty && c.lane < nw) grec[c.L.o_over + c.lane] = v_over;
#pragma unroll
      for (int s = 0; s < NSL; s++) {
        const int n = ((dirty_full >> s) & 1u) ? c.L.slot_words : M3_SLOT_HDR;
        if (s < n_slots && ((dm >> s) & 1u) && c.lane < n) grec[c.L.o_slots + s * c.L.slot_words + c.lane] = v_slot[s];
      }
    } else {
      if (edited) {  // the tile bits, one column mask, the changed rows of the move table
        for (int i = c.lane; i < nw; i += 64) grec[i] = c.dirt[i];
        if (c.lane == 0) grec[c.L.o_col + col_word] = E.rec[c.L.o_col + col_word];
        if (mv_chg) ((uint2 *)(grec + c.L.o_mv))[mv_cell] = ((const uint2 *)(E.rec + c.L.o_mv))[mv_cell];
      }
      if (over_dirty)  // new statistics: the overlay
        for (int i = c.lane; i < nw; i += 64) grec[c.L.o_over + i] = c.over[i];
      for (int s = 0; s < n_slots; s++) {
        if ((((dirty_hdr | dirty_full) >> s) & 1u) == 0u) continue;
        const int o0 = c.L.o_slots + s * c.L.slot_words;
        const int n = ((dirty_full >> s) & 1u) ? c.L.slot_words : M3_SLOT_HDR;
        for (int i = c.lane; i < n; i += 64) grec[o0 + i] = E.rec[o0 + i];
      }
    }
    if (any_reset && c.lane == 0) {
      rr.store(p.rng[env].rep);
      rp.store(p.rng[env].prob);
    }
    if (c.lane == 0) {
      S->pos[0] = pos[0];
      S->pos[1] = pos[1];
      S->pos[2] = pos[2];
      S->n_step = n_step;
      S->flags = flags;
      if (!upd_exit) {
        trg.write_ctrl_obs(p, env, st);
        trg.commit(p, env);
        S->iteration = iteration;
        S->changes = changes;
        S->last_loss = last_loss;
        S->ep_return = ep_return;
        for (int k = 0; k < NS; k++) S->stats[k] = st[k];
      }
    }
    PHASE_FLUSH();
  }
}

// launcher of one representation's kernels.  Compile-time cubes: 7^3 (BASELINE's) and 15^3 (the reference's stock map);
// turtle needs their 2 * DIM windows as well, wide's observation is the map.
template <int REP>
static hipError_t launch_3d_rep(KernelId id, const Params &p, int cpl, hipStream_t s) {
  const dim3 grid(p.n_envs), block(64);
  auto cube = [&](int d) {
    const bool dims = p.cfg.dims[0] == d && p.cfg.dims[1] == d && p.cfg.dims[2] == d;
    const bool win = REP == PCGRL_REP_WIDE || (p.cfg.obs_window[0] == 2 * d && p.cfg.obs_window[1] == 2 * d && p.cfg.obs_window[2] == 2 * d);
    return dims && win;
  };
  const int sc = m3_size_class(p.cfg.dims[0], p.cfg.dims[1], p.cfg.dims[2]);
  switch (id) {
    case K_STEP:
      if (cube(7))
        hipLaunchKernelGGL((r3_kernel<M3_STEP, 0, REP, 7>), grid, dim3(192), 0, s, p, cpl);
      else if (cube(15))
        hipLaunchKernelGGL((r3_kernel<M3_STEP, 1, REP, 15>), grid, dim3(64 * (2 + m3_observers<1>())), 0, s, p, cpl);
      else if (sc == 0)
        hipLaunchKernelGGL((r3_kernel<M3_STEP, 0, REP>), grid, dim3(64 * (2 + m3_observers<0>())), 0, s, p, cpl);
      else
        hipLaunchKernelGGL((r3_kernel<M3_STEP, 1, REP>), grid, dim3(64 * (2 + m3_observers<1>())), 0, s, p, cpl);
      break;
    case K_ROLLOUT:
      if (cube(7))
        hipLaunchKernelGGL((r3_kernel<M3_ROLLOUT, 0, REP, 7>), grid, block, 0, s, p, cpl);
      else if (sc == 0)
        hipLaunchKernelGGL((r3_kernel<M3_ROLLOUT, 0, REP>), grid, block, 0, s, p, cpl);
      else
        hipLaunchKernelGGL((r3_kernel<M3_ROLLOUT, 1, REP>), grid, block, 0, s, p, cpl);
      break;
    case K_RESET:
      if (sc == 0)
        hipLaunchKernelGGL((r3_kernel<M3_RESET, 0, REP>), grid, block, 0, s, p, cpl);
      else
        hipLaunchKernelGGL((r3_kernel<M3_RESET, 1, REP>), grid, block, 0, s, p, cpl);
      break;
    case K_OBSERVE:
      if (sc == 0)
        hipLaunchKernelGGL((r3_kernel<M3_OBSERVE, 0, REP>), grid, block, 0, s, p, cpl);
      else
        hipLaunchKernelGGL((r3_kernel<M3_OBSERVE, 1, REP>), grid, block, 0, s, p, cpl);
      break;
    default: return launch_3d(id, p, cpl, s);  // get_state, stats_for_grids, last_episode: no representation in them
  }
  return hipGetLastError();
}

#endif  // PCGRL_KERNEL_TU

}  // namespace pcgrl
