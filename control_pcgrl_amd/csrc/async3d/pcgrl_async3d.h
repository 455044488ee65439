// async3d/pcgrl_async3d.h -- gfx950 kernels for asynchronous stepping of minecraft_3D_maze (narrow representation):
// pcgrl_step_ready / pcgrl_reset / pcgrl_set_state / pcgrl_refresh_stats while a solver budget is set
// (include/pcgrl_amd_async3d.h has the contract).
//
// A synchronous launch (m3_kernel, pcgrl_kernels3d.h) lasts as long as its slowest env: the one whose edit dropped a cached
// pair of path searches.  Here a launch gives every env `budget` SEARCH TRIPS -- iterations of the loop of helper_3D.
// run_dijkstra (:422-490) as m3_search runs it: one trip pops one queue entry (short queues) or up to 16 (the wide trip) --
// summed over all the searches the env's step needs.  A search that has not ended when the budget is used up is PARKED
// between two trips and goes on in the next launch, where the loop bodies pop, accept and push exactly as m3_search's do:
// the budget only bounds the trip count, so every result is the synchronous kernels' (and the reference's).
//
// NO SPECULATION.  The synchronous step kernel runs the second search of a pair on a helper wave from a guessed root, which
// makes the number of trips an env's wave runs depend on whether the guess was right.  These kernels have no helper wave:
// both searches of a pair run one after the other on the simulate wave, so which launch an env advances in depends on the
// map, the action and the budget alone (capturable in a HIP graph: a replay equals the eager launches).
//
// Waves of a step workgroup (one workgroup per env): 0 simulate, 1 .. NOBS observe.  The observe waves are the synchronous
// kernel's: the observation shows the overlay of the PREVIOUS statistics update, so it does not depend on the searches, and
// the row of a busy env holds the observation of its step in flight.
//
// PARK RECORD (HBM, one per env, Params::soko -- null on a 3-D engine otherwise; written only by envs that park, read only
// by envs that resume).  32-bit words:
//   [0, 16)      valid, head, tail, n_order, epoch, trip, the entry in hand (2 words + flag), slot and search of the pair
//                that were running, farthest cell and plane marks of the pair's first search
//   tiles        the tile bits of the map the search belongs to (AFTER the pending edit): the record's identity
//   slots        the env's cached start planes as they were when the search parked (slots filled earlier in the same step
//                are kept with the parked step, not recomputed; nothing of an unfinished step is in the env's own record)
//   racc, best, info, order, ent   M3Work<SC>: accepted cells of the pair, per-cell tables, first-insertion order, queue ring
// Size class 0 (planes of <= 64 cells): 3 080 words = 12 320 bytes per env; size class 1 (up to 16^3): 26 440 words =
// 105 760 bytes per env.  A launch moves only what is live (n_cells entries of the tables, ring[head, tail)).
// A search is resumed only when the record is valid AND its tile bits equal the env's map; every reset (pcgrl_reset,
// pcgrl_set_state, pcgrl_refresh_stats) and pcgrl_import_state invalidates the records of the envs it covers, so a step
// abandoned that way starts over.  Results never depend on parked state.
#pragma once
#include <hip/hip_runtime.h>

#include "../pcgrl_dispatch.h"
#include "../pcgrl_kernels3d.h"

namespace pcgrl {

hipError_t launch_3d_async(KernelId id, const Params &p, int cpl, hipStream_t s);
// clears the valid word of the park records of the envs `mask` covers (null: all)
hipError_t launch_3d_async_unpark(void *pool, int Z, int Y, int X, int n_envs, const uint8_t *mask, hipStream_t s);

template <int SC>
struct A3P {  // word offsets inside a park record
  static constexpr int HDR = 16;
  static constexpr int O_TILES = HDR;
  static constexpr int O_SLOTS = O_TILES + M3C<SC>::NW;
  static constexpr int O_RACC = O_SLOTS + M3C<SC>::SLOTS * (M3_SLOT_HDR + 2 * M3C<SC>::NW);
  static constexpr int O_BEST = O_RACC + M3C<SC>::NW;
  static constexpr int O_INFO = O_BEST + 2 * M3C<SC>::CELLS;
  static constexpr int O_ORDER = O_INFO + M3C<SC>::CELLS;
  static constexpr int O_ENT = O_ORDER + M3C<SC>::CELLS / 2;
  static constexpr int WORDS = O_ENT + 2 * M3C<SC>::RING;
};
static_assert(A3P<0>::WORDS == 3080 && A3P<1>::WORDS == 26440, "park record sizes quoted in the headers and DESIGN.md");
inline size_t a3_park_bytes(int Z, int Y, int X) {
  return (size_t)(m3_size_class(Z, Y, X) == 0 ? A3P<0>::WORDS : A3P<1>::WORDS) * sizeof(uint32_t);
}

#ifdef PCGRL_KERNEL_TU

// a search between two trips (everything wave-uniform)
struct A3Q {
  int head, tail, n_order;
  uint32_t exv, eyv;  // the entry in hand (m3_search's scalar entry)
  int in_hand;
};
// the candidate walk between two trips of one of its searches
struct A3Walk {
  bool resume;  // in: a parked search of this map is in W / q
  int slot, stage, far1;
  uint32_t mk;
  A3Q q;
};

// m3_search's prologue: a new epoch, the root in hand
template <int SC>
__device__ inline void a3_begin(M3Work<SC> &W, const M3Ctx &c, int root, uint32_t &epoch, A3Q &q) {
  uint32_t ep = (uint32_t)__builtin_amdgcn_readfirstlane((int)epoch) + 1u;
  if (ep > 255u) {  // wrapped: clear the table once
    for (int i = c.lane; i < c.n_cells; i += 64) W.best[i].x = 0;
    ep = 1;
  }
  epoch = (uint32_t)__builtin_amdgcn_readfirstlane((int)ep);
  q.head = q.tail = q.n_order = 0;
  q.exv = (uint32_t)root | (0x1FFFu << 12);
  q.eyv = 1u;
  q.in_hand = 1;
}

// m3_search's loop (see there for why a trip of 16 entries is exact), bounded: every trip counts one unit of `used`, and
// the search returns false -- between two trips, its state in q -- when used has reached budget.  true: the search has
// ended (q.n_order accepted cells in W.order) or overflowed.
template <int SC>
__device__ inline bool a3_run(M3Work<SC> &W, const M3Ctx &c, A3Q &q, uint32_t epoch, uint32_t &trip, bool &overflow, int &used,
                              int budget) {
  constexpr int RING = M3C<SC>::RING, RM = RING - 1;
  const int16_t *mv = c.mv;
  const uint32_t ep = (uint32_t)__builtin_amdgcn_readfirstlane((int)epoch);
  uint32_t tr = (uint32_t)__builtin_amdgcn_readfirstlane((int)trip);
  int head = q.head, tail = q.tail, n_order = q.n_order;
  const int slot_i = c.lane >> 2, d = c.lane & 3;
  const uint32_t ep24 = ep << 24;
  uint32_t exv = q.exv, eyv = q.eyv;
  bool in_hand = q.in_hand != 0;
  bool ended = true;
  constexpr int WIDE_MIN = 2;
  for (;;) {
    if (!in_hand) {
      head = __builtin_amdgcn_readfirstlane(head);
      tail = __builtin_amdgcn_readfirstlane(tail);
      if (head >= tail) break;
    }
    if (__builtin_amdgcn_readfirstlane(used) >= budget) {  // parked here: between two trips
      ended = false;
      break;
    }
    used++;
    if (!in_hand && tail - head < WIDE_MIN) {  // a short queue is popped like the reference pops it
      const uint2 e = W.ent[head & RM];
      exv = e.x;
      eyv = e.y;
      head++;
      in_hand = true;
    }
    if (in_hand) {
      // ---- one entry: everything about it is scalar
      const uint32_t ex = (uint32_t)__builtin_amdgcn_readfirstlane((int)exv), ey = (uint32_t)__builtin_amdgcn_readfirstlane((int)eyv);
      const int cell = (int)(ex & 0xFFFu), parent = (int)((ex >> 12) & 0x1FFFu);
      const uint32_t len = ey;
      const uint32_t bxv = W.best[cell].x;
      const int mvl = mv[cell * 4 + d];
      const uint32_t bx = (uint32_t)__builtin_amdgcn_readfirstlane((int)bxv);
      const bool seen = (bx >> 24) == ep;
      in_hand = false;
      if (seen && (bx & 0xFFFFFFu) <= len) continue;  // :437-440 not shorter: dropped
      if (c.lane == 0) {
        if (!seen) W.order[n_order] = (uint16_t)cell;
        W.best[cell].x = ep24 | len;
        W.info[cell] = ex >> 12;
      }
      n_order += seen ? 0 : 1;
      const int m = c.lane < 4 ? mvl : 0;
      const int tcell = cell + (m >> 5);
      const bool ok = (m != 0) & (tcell != parent);
      const uint32_t okb = (uint32_t)M3_BALLOT(ok);
      const uint32_t cx = (uint32_t)tcell | ((uint32_t)cell << 12) | (((uint32_t)m & 31u) << 25) | ((uint32_t)d << 30);
      const uint32_t cy = len + ((uint32_t)m & 3u);
      if (okb == 0u) continue;
      head = __builtin_amdgcn_readfirstlane(head);
      tail = __builtin_amdgcn_readfirstlane(tail);
      if ((okb & (okb - 1u)) == 0u && head >= tail) {  // one successor and nothing waiting: it is the next entry
        const int l = __builtin_ctz(okb);
        exv = (uint32_t)__builtin_amdgcn_readlane((int)cx, l);
        eyv = (uint32_t)__builtin_amdgcn_readlane((int)cy, l);
        in_hand = true;
        continue;
      }
      const int npush = __popc(okb);
      if (tail + npush - head > RING) {
        overflow = true;
        break;
      }
      if (ok) W.ent[(tail + m3_below((uint64_t)okb)) & RM] = make_uint2(cx, cy);
      tail += npush;
      continue;
    }
    // ---- general trip: up to 16 entries
    tr++;
    const int n_q = tail - head;
    if (n_q > RING - 64) {  // (a trip pushes at most 64 entries)
      overflow = true;
      break;
    }
    const int nb = min(16, n_q);
    constexpr uint64_t D0 = 0x1111111111111111ull;  // the direction-0 lane of every entry
    const uint64_t live_m = M3_BALLOT(slot_i < nb);
    const int id = head + min(slot_i, nb - 1);
    const uint2 e = W.ent[id & RM];
    const int cell = (int)(e.x & 0xFFFu), parent = (int)((e.x >> 12) & 0x1FFFu);
    const uint32_t len = e.y;
    const uint32_t stamp = ((0x0FFFFFFFu - tr) << 4) | (uint32_t)slot_i;
    if (__builtin_amdgcn_inverse_ballot_w64(live_m & D0)) atomicMin(&W.best[cell].y, stamp);
    const uint2 b = W.best[cell];
    const int m = mv[cell * 4 + d];
    const uint32_t keyv = b.x ^ ep24;
    const uint64_t accept_m = M3_BALLOT(keyv > len) & live_m;
    const uint64_t dup_m = M3_BALLOT(b.y != stamp) & accept_m & D0;
    const int nproc = dup_m ? (__builtin_ctzll(dup_m) >> 2) : nb;
    const uint64_t doit_m = accept_m & M3_BALLOT(slot_i < nproc);
    const uint64_t acc0_m = doit_m & D0;
    const uint64_t first_m = acc0_m & M3_BALLOT(keyv >= (1u << 24));
    if (__builtin_amdgcn_inverse_ballot_w64(first_m)) W.order[n_order + m3_below(first_m)] = (uint16_t)cell;
    n_order += __popcll(first_m);
    if (__builtin_amdgcn_inverse_ballot_w64(acc0_m)) {
      W.best[cell].x = ep24 | len;
      W.info[cell] = e.x >> 12;
    }
    const int tcell = cell + (m >> 5);
    const uint32_t tlen = len + ((uint32_t)m & 3u);
    uint64_t ok_m = doit_m & M3_BALLOT(m != 0) & M3_BALLOT(tcell != parent);
    if (n_q > 32) {  // never queue what is known to be a no-op when popped
      const uint32_t bt = W.best[tcell].x ^ ep24;
      ok_m &= M3_BALLOT(bt > tlen);
    }
    if (__builtin_amdgcn_inverse_ballot_w64(ok_m))
      W.ent[(tail + m3_below(ok_m)) & RM] =
          make_uint2((uint32_t)tcell | ((uint32_t)cell << 12) | (((uint32_t)m & 31u) << 25) | ((uint32_t)d << 30), tlen);
    tail += __popcll(ok_m);
    head += nproc;
  }
  trip = tr;
  q.head = __builtin_amdgcn_readfirstlane(head);
  q.tail = __builtin_amdgcn_readfirstlane(tail);
  q.n_order = __builtin_amdgcn_readfirstlane(n_order);
  q.exv = (uint32_t)__builtin_amdgcn_readfirstlane((int)exv);
  q.eyv = (uint32_t)__builtin_amdgcn_readfirstlane((int)eyv);
  q.in_hand = in_hand ? 1 : 0;
  return ended;
}

// m3_fill_slot without the helper wave, resumable: the pair of searches of one start candidate -> slot s.
// false: parked (wk holds the pair's state); true: the slot is filled, or `overflow`.
template <int SC>
__device__ inline bool a3_fill_slot(M3Work<SC> &W, const M3Ctx &c, int s, int start_bit, int sz, uint32_t &epoch, uint32_t &trip,
                                    bool &overflow, A3Walk &wk, bool resume, int &used, int budget) {
  if (!resume) {
    if (c.lane == 0) c.hdr(s)->valid = 0;
    for (int i = c.lane; i < c.L.nw; i += 64) W.racc[i] = 0;
    a3_begin(W, c, sz * c.YX + start_bit, epoch, wk.q);
    wk.stage = 0;
    wk.slot = s;
  }
  if (wk.stage == 0) {
    if (!a3_run(W, c, wk.q, epoch, trip, overflow, used, budget)) return false;
    if (overflow) return true;
    wk.mk = m3_collect(W, c, wk.q.n_order, wk.far1);
    a3_begin(W, c, wk.far1, epoch, wk.q);
    wk.stage = 1;
  }
  if (!a3_run(W, c, wk.q, epoch, trip, overflow, used, budget)) return false;
  if (overflow) return true;
  int far2 = 0;
  (void)m3_collect(W, c, wk.q.n_order, far2);
  const int max_dist = (int)(__builtin_amdgcn_readfirstlane((int)W.best[far2].x) & 0xFFFF);
  const int n_jump = m3_path_tiles(W, c, s, far2);
  uint32_t *ra = c.racc(s);
  for (int i = c.lane; i < c.L.nw; i += 64) ra[i] = W.racc[i];
  if (c.lane == 0) {
    M3SlotHdr h;
    h.start = (uint16_t)start_bit;
    h.valid = 1;
    h.max_dist = (uint16_t)max_dist;
    h.n_jump = (uint16_t)n_jump;
    h.mk = wk.mk & ((1u << c.Z) - 1u);
    h.far1 = (uint32_t)(wk.far1 + 1) | ((uint32_t)(far2 + 1) << 16);
    *c.hdr(s) = h;
  }
  return true;
}

// m3_paths, resumable.  0: finished (st[1], st[2], c.over written); 1: parked (wk); 2: overflow.
// The walk always starts at the first candidate: slots filled before a park are valid in c.slots and are passed over.
template <int SC>
__device__ inline int a3_paths(M3Work<SC> &W, const M3Ctx &c, PM<M3C<SC>::PW> air, int32_t *st, uint32_t &epoch, uint32_t &trip,
                               uint32_t &filled, A3Walk &wk, int &used, int budget) {
  constexpr int PW = M3C<SC>::PW;
  const PM<PW> above = pm_down(air), below = pm_up(air);
  const PM<PW> cand = (c.lane >= 1 && c.lane + 1 < c.Z) ? (air & above & ~below) : pm_zero<PW>();
  uint32_t marked = 0;
  int final_value = 0, n_jump = 0, best_slot = -1;
  bool overflow = false;
  while (true) {
    const bool mine = c.lane < c.Z && pm_any(cand) && !((marked >> c.lane) & 1u);
    const uint64_t b = M3_BALLOT(mine);
    if (b == 0) break;
    const int sz = __builtin_ctzll(b);
    const int bit = __builtin_amdgcn_readlane(pm_ctz(cand), sz);
    const int s = sz - 1;
    {
      const uint32_t h0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)*(const uint32_t *)c.hdr(s));  // start | valid << 16
      if (!((h0 >> 16) != 0u && (int)(h0 & 0xFFFFu) == bit)) {
        const bool resume = wk.resume && wk.slot == s;
        wk.resume = false;  // (a parked pair is either the first one the walk needs or not of this map's walk)
        const bool ended = a3_fill_slot(W, c, s, bit, sz, epoch, trip, overflow, wk, resume, used, budget);
        filled |= 1u << s;
        if (!ended) return 1;
        if (overflow) return 2;
      }
    }
    const uint32_t h1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((const uint32_t *)c.hdr(s))[1]);  // max_dist | n_jump << 16
    marked |= (uint32_t)__builtin_amdgcn_readfirstlane((int)c.hdr(s)->mk);
    n_jump = (int)(h1 >> 16);  // :553 overwritten by every processed component
    if ((int)(h1 & 0xFFFFu) > final_value) {
      final_value = (int)(h1 & 0xFFFFu);
      best_slot = s;
    }
  }
  // remove_stacked_path_tiles (:657-675) then the transposed overlay of process_observation (:84-93), as m3_paths
  for (int i = c.lane; i < c.L.nw; i += 64) c.over[i] = 0;
  if (best_slot >= 0) {
    const uint32_t *pathm = c.spath(best_slot);
    bool by_rows = false;
    if constexpr (SC == 0) by_rows = c.X <= 8 && c.Z * c.Y <= 64;
    if (by_rows) {
      const int r = c.lane, z = r / c.Y, y = r - z * c.Y;
      if (r < c.Z * c.Y) {
        auto row_at = [&](int o) -> uint32_t {  // X bits from bit offset o of the mask
          const int w0 = o >> 5, w1 = w0 + 1 < c.L.nw ? w0 + 1 : w0;
          const uint64_t v = (uint64_t)pathm[w0] | ((uint64_t)pathm[w1] << 32);
          return (uint32_t)(v >> (o & 31)) & ((1u << c.X) - 1u);
        };
        const int o = r * c.X;
        uint32_t keep = row_at(o);
        if (z >= 1) keep &= ~row_at(o - c.YX);
        if (z < c.X) {
          for (int x = 0; x < c.X && x < c.Z; x++) {
            const int oi = (x * c.Y + y) * c.X + z;
            if ((keep >> x) & 1u) atomicOr(&c.over[oi >> 5], 1u << (oi & 31));
          }
        }
      }
    } else {
      const PM<PW> P = c.lane < c.Z ? m3_plane_bits<PW>(pathm, c, c.lane) : pm_zero<PW>();
      PM<PW> keep = P & ~pm_up(P);
      const int z = c.lane;
      while (M3_BALLOT(pm_any(keep)) != 0) {
        if (pm_any(keep)) {
          const int q = pm_ctz(keep);
          keep = keep & ~pm_lowest(keep);
          const int y = q / c.X, x = q - y * c.X;
          if (x < c.Z && z < c.X) {
            const int oi = (x * c.Y + y) * c.X + z;
            atomicOr(&c.over[oi >> 5], 1u << (oi & 31));
          }
        }
      }
    }
  }
  st[1] = final_value;
  st[2] = n_jump;
  return 0;
}

// ---------------------------------------------------------------------------------------------- park records
__device__ inline void a3_copy_words(uint32_t *dst, const uint32_t *src, int n, int lane) {  // both 16-byte aligned
  const int n4 = (n + 3) >> 2;  // (every table's capacity is a multiple of 4 words)
  for (int i = lane; i < n4; i += 64) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
}

template <int SC>
__device__ inline void a3_park_save(uint32_t *pr, M3Work<SC> &W, const M3Ctx &c, const A3Walk &wk, uint32_t epoch, uint32_t trip) {
  using P = A3P<SC>;
  constexpr int RM = M3C<SC>::RING - 1;
  if (c.lane == 0) {
    pr[1] = (uint32_t)wk.q.head;
    pr[2] = (uint32_t)wk.q.tail;
    pr[3] = (uint32_t)wk.q.n_order;
    pr[4] = epoch;
    pr[5] = trip;
    pr[6] = wk.q.exv;
    pr[7] = wk.q.eyv;
    pr[8] = (uint32_t)wk.q.in_hand;
    pr[9] = (uint32_t)wk.slot;
    pr[10] = (uint32_t)wk.stage;
    pr[11] = (uint32_t)wk.far1;
    pr[12] = wk.mk;
    pr[0] = 1u;
  }
  a3_copy_words(pr + P::O_TILES, c.dirt, c.L.nw, c.lane);
  for (int i = c.lane; i < c.L.n_slots * c.L.slot_words; i += 64) pr[P::O_SLOTS + i] = c.slots[i];
  a3_copy_words(pr + P::O_RACC, W.racc, c.L.nw, c.lane);
  a3_copy_words(pr + P::O_BEST, (const uint32_t *)W.best, 2 * c.n_cells, c.lane);
  a3_copy_words(pr + P::O_INFO, W.info, c.n_cells, c.lane);
  a3_copy_words(pr + P::O_ORDER, (const uint32_t *)W.order, (wk.q.n_order + 1) >> 1, c.lane);
  for (int i = wk.q.head + c.lane; i < wk.q.tail; i += 64) ((uint2 *)(pr + P::O_ENT))[i & RM] = W.ent[i & RM];
}

// true: the record holds a parked search of exactly the map in c.dirt; W, c.slots, wk, epoch, trip are then its state
template <int SC>
__device__ inline bool a3_park_load(const uint32_t *pr, M3Work<SC> &W, const M3Ctx &c, A3Walk &wk, uint32_t &epoch, uint32_t &trip) {
  using P = A3P<SC>;
  constexpr int RM = M3C<SC>::RING - 1;
  bool same = pr[0] == 1u;
  for (int i = c.lane; i < c.L.nw; i += 64) same = same && pr[P::O_TILES + i] == c.dirt[i];
  if (M3_BALLOT(!same) != 0) return false;
  wk.q.head = __builtin_amdgcn_readfirstlane((int)pr[1]);
  wk.q.tail = __builtin_amdgcn_readfirstlane((int)pr[2]);
  wk.q.n_order = __builtin_amdgcn_readfirstlane((int)pr[3]);
  epoch = (uint32_t)__builtin_amdgcn_readfirstlane((int)pr[4]);
  trip = (uint32_t)__builtin_amdgcn_readfirstlane((int)pr[5]);
  wk.q.exv = (uint32_t)__builtin_amdgcn_readfirstlane((int)pr[6]);
  wk.q.eyv = (uint32_t)__builtin_amdgcn_readfirstlane((int)pr[7]);
  wk.q.in_hand = __builtin_amdgcn_readfirstlane((int)pr[8]);
  wk.slot = __builtin_amdgcn_readfirstlane((int)pr[9]);
  wk.stage = __builtin_amdgcn_readfirstlane((int)pr[10]);
  wk.far1 = __builtin_amdgcn_readfirstlane((int)pr[11]);
  wk.mk = (uint32_t)__builtin_amdgcn_readfirstlane((int)pr[12]);
  // (a record is only ever written by a3_park_save, so these are in range; the clamps keep a corrupt one inside LDS)
  if (wk.q.tail - wk.q.head > M3C<SC>::RING || wk.q.tail < wk.q.head || wk.q.n_order > c.n_cells || wk.q.n_order < 0 ||
      (unsigned)wk.slot >= (unsigned)c.L.n_slots || (unsigned)wk.far1 >= (unsigned)c.n_cells)
    return false;
  for (int i = c.lane; i < c.L.n_slots * c.L.slot_words; i += 64) c.slots[i] = pr[P::O_SLOTS + i];
  a3_copy_words(W.racc, pr + P::O_RACC, c.L.nw, c.lane);
  a3_copy_words((uint32_t *)W.best, pr + P::O_BEST, 2 * c.n_cells, c.lane);
  a3_copy_words(W.info, pr + P::O_INFO, c.n_cells, c.lane);
  a3_copy_words((uint32_t *)W.order, pr + P::O_ORDER, (wk.q.n_order + 1) >> 1, c.lane);
  for (int i = wk.q.head + c.lane; i < wk.q.tail; i += 64) W.ent[i & RM] = ((const uint2 *)(pr + P::O_ENT))[i & RM];
  wk.resume = true;
  return true;
}

__global__ __launch_bounds__(256) void a3_unpark_kernel(uint32_t *pool, int words, int n_envs, const uint8_t *mask) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n_envs && (mask == nullptr || mask[e] != 0)) pool[(size_t)e * words] = 0u;
}

// ---------------------------------------------------------------------------------------------- kernels
// STEP: pcgrl_step_ready (waves: simulate, observe x NOBS); !STEP: pcgrl_reset / pcgrl_set_state / pcgrl_refresh_stats (one wave).
// DIM: cubic map with its 2 DIM window as compile-time dimensions (7, 15), 0: run-time dimensions.
template <bool STEP, int SC, int DIM = 0>
__global__ __launch_bounds__(STEP ? 64 * (1 + m3_observers<SC>()) : 64, (STEP && SC == 0) ? 4 : 1)
void a3_kernel(Params p, int cpl) {
  constexpr int PW = M3C<SC>::PW, NS = M3_NS, NOBS = m3_observers<SC>();
  if (STEP) touch_kernarg(p);
  __shared__ M3Env<SC> E;
  __shared__ __attribute__((aligned(16))) M3Work<SC> W;
  __shared__ int32_t obs_read;  // observe waves that hold their copy of the old state
  __shared__ M3ObsLds<SC> O;
  M3Ctx c;
  c.lane = (int)__lane_id();
  c.Z = DIM ? DIM : p.cfg.dims[0];
  c.Y = DIM ? DIM : p.cfg.dims[1];
  c.X = DIM ? DIM : p.cfg.dims[2];
  if (DIM) cpl = (DIM * DIM * DIM + 63) / 64;
  c.YX = c.Y * c.X;
  c.n_cells = c.Z * c.YX;
  c.L = m3_layout(c.Z, c.Y, c.X);
  c.dirt = E.rec;
  c.over = E.rec + c.L.o_over;
  c.col = (uint16_t *)(E.rec + c.L.o_col);
  c.slots = E.rec + c.L.o_slots;
  c.mv = (int16_t *)(E.rec + c.L.o_mv);
  const int nw = c.L.nw, n_slots = c.L.n_slots;
  const int env = blockIdx.x;
  const int budget = p.sk_budget;
  uint32_t *grec = (uint32_t *)p.planes + (size_t)env * c.L.rec_words;
  uint32_t *park = (uint32_t *)p.soko + (size_t)env * A3P<SC>::WORDS;
  EnvState *S = &p.st[env];

  if constexpr (STEP) {
    if (threadIdx.x == 0) obs_read = 0;
    __syncthreads();
    const int wave_id = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave_id >= 1) {
      // ------------------------------------------------------------------------------------------ observe wave (m3_kernel's)
      if (p.obs == nullptr) return;
      const int part = wave_id - 1;
      uint32_t *obits = O.bits[part];
      for (int i = c.lane; i < 2 * nw; i += 64) obits[i] = grec[i];
      int pos[3] = {S->pos[0], S->pos[1], S->pos[2]};
      int n_step = S->n_step, iteration = S->iteration, changes = S->changes;
      const int flags = S->flags;
      const int new_action = p.actions[env], pend_action = S->pend_action;
      Pcg rp, rr;
      rp.load(p.rng[env].prob);
      rr.load(p.rng[env].rep);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (c.lane == 0) __hip_atomic_fetch_add(&obs_read, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      uint32_t *odirt = obits, *oover = obits + nw;
      if (flags & ENV_PENDING_STATS) {  // a reset map that waits for its statistics: the first observation of the episode
        m3_encode_obs<2 * DIM>(odirt, oover, c, p, env, pos, false, O.rows, (int)(sizeof(O.rows) / sizeof(uint2)), nullptr, part, NOBS);
        return;
      }
      const int action = (flags & ENV_PENDING_STEP) ? pend_action : new_action;  // the step in flight
      iteration += 1;
      bool change = false;
      if (action >= 0 && action < 2) {
        const int ci = m3_cell(c, pos[2], pos[1], pos[0]);  // pos = (z, y, x)
        change = m3_bit(odirt, ci) != (action != 0);
        if (change && c.lane == 0) odirt[ci >> 5] ^= 1u << (ci & 31);
        m3_advance_pos(c, pos, n_step);
      }
      changes += change ? 1 : 0;
      bool done = iteration > p.cfg.max_iterations;
      if (p.cfg.max_changes >= 0) done = done || changes > p.cfg.max_changes;
      if (done && p.auto_reset != 0) {  // first observation of the new episode: no overlay (PcgrlEnv.reset)
        m3_reset_rng(odirt, c, p, cpl, rp, rr);
        pos[0] = pos[1] = pos[2] = 0;
        m3_encode_obs<2 * DIM>(odirt, oover, c, p, env, pos, false, O.rows, (int)(sizeof(O.rows) / sizeof(uint2)), nullptr, part, NOBS);
      } else {
        m3_encode_obs<2 * DIM>(odirt, oover, c, p, env, pos, true, O.rows, (int)(sizeof(O.rows) / sizeof(uint2)), nullptr, part, NOBS);
      }
      return;
    }
    __builtin_amdgcn_s_setprio(3);
  }

  // ---------------------------------------------------------------------------------------------- simulate wave
  uint32_t epoch = 0, trip = 0;
  uint32_t dirty_hdr = 0, dirty_full = 0;
  int used = 0;
  A3Walk wk;
  wk.resume = false;
  wk.slot = wk.stage = wk.far1 = 0;
  wk.mk = 0;
  wk.q = A3Q{0, 0, 0, 0u, 0u, 0};
  auto init_work = [&]() {
    for (int i = c.lane; i < c.n_cells; i += 64) W.best[i] = make_uint2(0u, 0xFFFFFFFFu);
  };
  PM<PW> notx0, notxl;
  m3_edge_masks<PW>(p, notx0, notxl);
  auto plane_of = [&](const uint32_t *dirt) { return c.lane < c.Z ? m3_plane_air<PW>(dirt, c, c.lane) : pm_zero<PW>(); };
  // a map the record's tables do not belong to: columns, move table, no cached slots
  auto fresh_tables = [&]() {
    const PM<PW> air = plane_of(c.dirt);
    for (int i = c.lane; i < c.L.o_slots - c.L.o_col; i += 64) E.rec[c.L.o_col + i] = 0;
    m3_build_cols<PW>(c, air);
    m3_build_moves(c);
    if (c.lane < n_slots) *(uint4 *)c.hdr(c.lane) = make_uint4(0u, 0u, 0u, 0u);
  };
  auto store_record = [&]() {
    for (int i = c.lane; i < c.L.rec_words / 4; i += 64) ((uint4 *)grec)[i] = ((const uint4 *)E.rec)[i];
  };
  // the statistics of the final map in E.rec (tables in place) from scratch, within what is left of the budget.
  // 0: st is complete; 1: parked (record saved); 2: overflow (st[0] only)
  auto fresh_stats = [&](int32_t *st) -> int {
    const PM<PW> air = plane_of(c.dirt);
    const int r = a3_paths<SC>(W, c, air, st, epoch, trip, dirty_full, wk, used, budget);
    if (r == 1) {
      a3_park_save<SC>(park, W, c, wk, epoch, trip);
      return 1;
    }
    st[0] = m3_regions<PW>(c, air, notx0, notxl);
    return r;
  };
  auto wait_observers = [&]() {
    if (STEP && p.obs != nullptr) {
      while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&obs_read, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != NOBS)
        __builtin_amdgcn_s_sleep(1);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
  };

  int32_t st[NS] = {0, 0, 0};
  EnvTargets<NS> trg;
  Pcg rp, rr;

  if constexpr (!STEP) {
    if (p.mask != nullptr && p.mask[env] == 0) return;
    const int flags0 = S->flags;
    if (p.refresh_only && (flags0 & ENV_PENDING_STEP)) {  // a parked step is left as it is: the statistics of the current map
      if (c.lane == 0 && p.stats_out)
        for (int k = 0; k < NS; k++) p.stats_out[(size_t)env * NS + k] = S->stats[k];
      return;
    }
    for (int i = c.lane; i < 2 * nw; i += 64) E.rec[i] = grec[i];
    for (int k = 0; k < NS; k++) st[k] = S->stats[k];
    init_work();
    if (c.lane == 0) park[0] = 0u;  // whatever was parked for this env is abandoned (a3_park_save sets it again)
    if (p.refresh_only) {
      trg.load(p, env, false);
      fresh_tables();
      const int r = fresh_stats(st);
      if (r == 2 && c.lane == 0) atomicOr(p.err, 4);
      store_record();
      if (c.lane == 0) {
        if (r == 1) {
          S->flags = ENV_PENDING_STATS;
        } else {
          S->last_loss = trg.loss(p.cfg, st);
          S->flags = 0;
          for (int k = 0; k < NS; k++) {
            S->stats[k] = st[k];
            if (p.stats_out) p.stats_out[(size_t)env * NS + k] = st[k];
          }
        }
      }
      return;
    }
    int pos[3] = {0, 0, 0};
    if (p.init_grids) {
      m3_load_bytes(c.dirt, c, p.init_grids + (size_t)env * c.n_cells);
      if (p.init_pos)
        for (int d = 0; d < 3; d++) pos[d] = p.init_pos[(size_t)env * 3 + d];
    } else {
      rp.load(p.rng[env].prob);
      rr.load(p.rng[env].rep);
      m3_reset_rng(c.dirt, c, p, cpl, rp, rr);
      if (c.lane == 0) {
        rr.store(p.rng[env].rep);
        rp.store(p.rng[env].prob);
      }
    }
    fresh_tables();
    const int r = fresh_stats(st);
    int n_step = 0, iteration = 0, changes = 0;
    double ep_return = 0.0;
    if (p.set_state) {
      if (p.in_counters) {
        iteration = p.in_counters[(size_t)env * 4 + 0];
        changes = p.in_counters[(size_t)env * 4 + 1];
        n_step = p.in_counters[(size_t)env * 4 + 2];
      }
      if (p.in_ep_return) ep_return = p.in_ep_return[env];
    }
    trg.load(p, env, true);
    if (r == 2 && c.lane == 0) atomicOr(p.err, 4);
    store_record();
    if (c.lane == 0) {
      trg.commit(p, env);
      S->pos[0] = pos[0];
      S->pos[1] = pos[1];
      S->pos[2] = pos[2];
      S->n_step = n_step;
      S->iteration = iteration;
      S->changes = changes;
      S->ep_return = ep_return;
      if (r == 1) {
        S->flags = ENV_PENDING_STATS;  // statistics and last_loss arrive with a later pcgrl_step_ready launch
      } else {
        S->flags = 0;
        S->last_loss = trg.loss(p.cfg, st);
        for (int k = 0; k < NS; k++) S->stats[k] = st[k];
      }
    }
    return;
  } else {
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
    const int new_action = p.actions[env], pend_action = S->pend_action;
    const bool pend_step = (flags & ENV_PENDING_STEP) != 0, pend_stats = (flags & ENV_PENDING_STATS) != 0;
    const int action = pend_step ? pend_action : new_action;
    trg.load(p, env, false);
    if (SC == 0) {
#pragma unroll
      for (int k = 0; k < CH; k++) {
        const int i = c.lane + 64 * k;
        if (i < c.L.rec_words / 4) ((uint4 *)E.rec)[i] = rch[k];
      }
    } else {
      // size class 1: tile bits, overlay and column masks first; the tables only for a step that needs statistics
      const int s0 = (c.L.o_slots & ~3) / 4, s1 = c.L.rec_words / 4;
      m3_copy_batched<4>((uint4 *)E.rec, (const uint4 *)grec, 0, s0, c.lane);
      const bool ok0 = action >= 0 && action < 2;
      const bool ch0 = ok0 && m3_bit(c.dirt, m3_cell(c, pos[2], pos[1], pos[0])) != (action != 0);
      const bool reset0 = p.auto_reset != 0 && iteration + 1 > p.cfg.max_iterations;
      if (pend_stats || ch0 || reset0) m3_copy_batched<16>((uint4 *)E.rec, (const uint4 *)grec, s0, s1, c.lane);
    }
    uint8_t status = 0;

    if (pend_stats) {
      // ---- a reset map (the record's tables are its own) whose statistics wait for a parked search: no action is taken
      if (!a3_park_load<SC>(park, W, c, wk, epoch, trip)) init_work();
      const int r = fresh_stats(st);
      if (r == 1) {
        if (c.lane == 0) p.ready[env] = PCGRL_ENV_BUSY;
        return;  // (everything the walk has done so far is in the park record)
      }
      if (r == 2 && c.lane == 0) atomicOr(p.err, 4);
      wait_observers();
      store_record();
      if (c.lane == 0) {
        park[0] = 0u;
        S->flags = 0;
        S->last_loss = trg.loss(p.cfg, st);
        for (int k = 0; k < NS; k++) S->stats[k] = st[k];
        p.ready[env] = 0;
      }
      return;
    }

    // ---- step (envs/pcgrl_env.py:267-342 with narrow_rep.py:89-102), as m3_kernel
    bool whole_record = false, edited = false, mv_chg = false, over_dirty = false, ovf_any = false;
    int mv_cell = 0, col_word = 0;
    const bool bad = action < 0 || action >= 2;
    iteration += 1;
    bool change = false;
    int ex = 0, ey = 0, ez = 0;
    if (!bad) {
      ez = pos[0], ey = pos[1], ex = pos[2];  // pos = (z, y, x)
      const int ci = m3_cell(c, ex, ey, ez);
      const bool old = m3_bit(c.dirt, ci);
      change = old != (action != 0);
      if (change) {
        if (c.lane == 0) {
          const int q = ey * c.X + ex;
          atomicXor(&c.dirt[ci >> 5], 1u << (ci & 31));
          atomicXor((uint32_t *)c.col + (q >> 1), (1u << ez) << (16 * (q & 1)));
        }
        col_word = (ey * c.X + ex) >> 1;
        edited = true;
        dirty_hdr |= m3_update_moves(c, ex, ey, ez, mv_chg, mv_cell);
      }
      m3_advance_pos(c, pos, n_step);
    } else if (c.lane == 0 && !pend_step) {
      atomicOr(p.err, 1);
    }
    changes += change ? 1 : 0;
    bool done = iteration > p.cfg.max_iterations;
    if (p.cfg.max_changes >= 0) done = done || changes > p.cfg.max_changes;
    const bool do_reset = done && p.auto_reset != 0;
    if (change) {
      const PM<PW> air = plane_of(c.dirt);
      const int32_t st_old[NS] = {st[0], st[1], st[2]};
      // a step that waited: its parked search if the record is of exactly this map (E.rec's slots become those of the
      // parked step), else from the start.  Either way the whole record is written when the step completes.
      if (!(pend_step && a3_park_load<SC>(park, W, c, wk, epoch, trip))) init_work();
      whole_record = pend_step;
      const int r = a3_paths<SC>(W, c, air, st, epoch, trip, dirty_full, wk, used, budget);
      if (r == 1) {
        // nothing of the unfinished step is committed: the env's record stays the state before it
        a3_park_save<SC>(park, W, c, wk, epoch, trip);
        wait_observers();
        if (c.lane == 0) {
          if (!pend_step) {
            S->flags = flags | ENV_PENDING_STEP;
            S->pend_action = action;
          }
          p.ready[env] = PCGRL_ENV_BUSY;
        }
        return;
      }
      over_dirty = true;
      if (r == 2) {  // queue overflow, as m3_kernel: previous statistics, every cached plane dropped, the env marked stale
        for (int i = 0; i < NS; i++) st[i] = st_old[i];
        if (c.lane < n_slots) *(uint4 *)c.hdr(c.lane) = make_uint4(0u, 0u, 0u, 0u);
        dirty_hdr = (1u << n_slots) - 1u;
        flags |= ENV_STATS_DIRTY;
        ovf_any = true;
      } else {
        if (flags & ENV_STATS_DIRTY) {
          st[0] = m3_regions<PW>(c, air, notx0, notxl);
        } else {
          PM<PW> A = air;  // the planes without the edited cell
          if (c.lane == ez) {
            PM<PW> e = pm_zero<PW>();
            pm_set(e, ey * c.X + ex);
            A = A & ~e;
          }
          st[0] = m3_regions_update<PW>(c, A, notx0, notxl, ey * c.X + ex, ez, action == 0, st_old[0]);
        }
        flags &= ~ENV_STATS_DIRTY;
      }
    }
    flags &= ~ENV_PENDING_STEP;
    status = PCGRL_ENV_EMITTED;
    const double loss = trg.loss(p.cfg, st);
    const double rew = loss - last_loss;
    last_loss = loss;
    ep_return += rew;
    if (c.lane == 0) {
      if (p.reward) p.reward[env] = (float)rew;
      if (p.done) p.done[env] = done ? 1 : 0;
      if (p.stats_out)
        for (int i = 0; i < NS; i++) p.stats_out[(size_t)env * NS + i] = st[i];
    }
    bool any_reset = false;
    if (do_reset) {
      rp.load(p.rng[env].prob);
      rr.load(p.rng[env].rep);
      if (c.lane == 0) {  // (fields no observe wave reads)
        latch_episode<NS>(p, env, S, ep_return, iteration, st);
        accumulate_episode<NS>(S);
      }
      m3_reset_rng(c.dirt, c, p, cpl, rp, rr);
      any_reset = true;
      whole_record = true;
      pos[0] = pos[1] = pos[2] = 0;
      fresh_tables();
      if (!change) init_work();  // (else the step's own searches have set the tables up: epochs, as m3_kernel)
      wk.resume = false;
      const int r = fresh_stats(st);
      flags = 0;
      n_step = iteration = changes = 0;
      ep_return = 0.0;
      trg.load(p, env, true);
      if (r == 1) {  // the new episode's statistics wait for the parked search: EMITTED | BUSY
        flags = ENV_PENDING_STATS;
        status |= PCGRL_ENV_BUSY;
      } else {
        if (r == 2) ovf_any = true;
        last_loss = trg.loss(p.cfg, st);
      }
      if (c.lane == 0) trg.commit(p, env);
    }
    if (pend_step && !(status & PCGRL_ENV_BUSY) && c.lane == 0) park[0] = 0u;  // the parked step is complete, nothing new parked
    if (ovf_any && c.lane == 0) atomicOr(p.err, 4);
    // ---- write back, once the observe waves have read the old state
    wait_observers();
    if (whole_record) {
      store_record();
    } else {
      if (edited) {  // the tile bits, one column mask, the changed rows of the move table
        for (int i = c.lane; i < nw; i += 64) grec[i] = c.dirt[i];
        if (c.lane == 0) grec[c.L.o_col + col_word] = E.rec[c.L.o_col + col_word];
        if (mv_chg) ((uint2 *)(grec + c.L.o_mv))[mv_cell] = ((const uint2 *)(E.rec + c.L.o_mv))[mv_cell];
      }
      if (over_dirty)
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
      S->iteration = iteration;
      S->changes = changes;
      S->ep_return = ep_return;
      if (!(flags & ENV_PENDING_STATS)) {
        S->last_loss = last_loss;
        for (int k = 0; k < NS; k++) S->stats[k] = st[k];
      }
      p.ready[env] = status;
    }
  }
}

inline hipError_t launch_3d_async_impl(KernelId id, const Params &p, int cpl, hipStream_t s) {
  const dim3 grid(p.n_envs);
  auto cube = [&](int d) {
    return p.cfg.dims[0] == d && p.cfg.dims[1] == d && p.cfg.dims[2] == d && p.cfg.obs_window[0] == 2 * d &&
           p.cfg.obs_window[1] == 2 * d && p.cfg.obs_window[2] == 2 * d;
  };
  const int sc = m3_size_class(p.cfg.dims[0], p.cfg.dims[1], p.cfg.dims[2]);
  if (id == K_STEP) {
    if (cube(7))
      hipLaunchKernelGGL((a3_kernel<true, 0, 7>), grid, dim3(64 * (1 + m3_observers<0>())), 0, s, p, cpl);
    else if (cube(15))
      hipLaunchKernelGGL((a3_kernel<true, 1, 15>), grid, dim3(64 * (1 + m3_observers<1>())), 0, s, p, cpl);
    else if (sc == 0)
      hipLaunchKernelGGL((a3_kernel<true, 0>), grid, dim3(64 * (1 + m3_observers<0>())), 0, s, p, cpl);
    else
      hipLaunchKernelGGL((a3_kernel<true, 1>), grid, dim3(64 * (1 + m3_observers<1>())), 0, s, p, cpl);
  } else if (id == K_RESET) {
    if (sc == 0)
      hipLaunchKernelGGL((a3_kernel<false, 0>), grid, dim3(64), 0, s, p, cpl);
    else
      hipLaunchKernelGGL((a3_kernel<false, 1>), grid, dim3(64), 0, s, p, cpl);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

#endif  // PCGRL_KERNEL_TU

}  // namespace pcgrl
