// solutions/pcgrl_solutions.h -- Sokoban solutions on the device (include/pcgrl_amd_solutions.h): the move list behind
// `sol-length`, i.e. what SokobanProblem.get_stats leaves in stats["solution"] (sokoban_prob.py:178, _run_game :99-148).
//
// The rules:
//   precondition   exactly one player, crates == targets > 0, one region (sokoban_prob.py:172-177); otherwise the reference
//                  has no "solution" key: len = -1, dist-win = H * W * (H + W).
//   cascade        BFSAgent, then AStarAgent with balance 1, 0.5, 0, each limited to solver_power iterations; the first stage
//                  that pops a winning node ends it.  No stage wins: len = 0 (the reference returns []), dist-win = the
//                  heuristic of the last stage's best node.  (A BFS stage that runs its queue dry ends the cascade: see
//                  sk_cascade, pcgrl_sokoban.h.)
//   solution       Node.getActions (engine.py:27-35) of the winning node: the actions from the root down, one per level of
//                  depth.  Node.getChildren drops every child whose player did not move (engine.py:19-20), so a node's action is
//                  (px - parent.px, py - parent.py); it is handed out as its index in `directions` (engine.py:3): 0 = x-1,
//                  1 = x+1, 2 = y-1, 3 = y+1.
//
// The statistics kernels run the same cascade (sk_stage, pcgrl_sokoban.h) but return only (h, depth) of a win, and the node
// that won cannot be found afterwards: under A* several open nodes with h == 0 at that depth can exist and which one was
// popped depends on the heap order.  So this kernel carries a stage driver of its own, sol_stage: the loop of sk_stage in its
// plain form -- same pops, same pushes, same visited set, same iteration cap, built from the same pieces; no record requested
// ahead, no helper waves, no parking, no cancel -- which also yields the index of the popped node that won.  It is a second
// statement of one loop; tests/test_gpu_solutions.py pins the two against each other (sol-length, dist-win) on every level.
//
// One map per workgroup of one wavefront, on a locked slot of the engine's workspace pool (the protocol of sokoban_solve);
// the stages run one after the other on stage workspace 0 (levels with more than SK_MAXC pairs: the eight-register form,
// whose node crate lists spread over the crate areas of the slot's four workspaces, like sk_cascade<SK_NH_HUGE>).  The top of
// the A* open list lives in LDS (SK_LDS_HEAP entries), the rest in the workspace.  The walk back from the winner is a
// dependent chain of 16-byte loads, at most solver_power long; the -1 fill is written by all lanes.  Plain vector stores only.
#pragma once
#include <hip/hip_runtime.h>

#include "../pcgrl_common.h"

namespace pcgrl {

struct SolArgs {
  int8_t *moves;      // [n][cap]: the first min(len, cap) moves, root first; every later byte is -1
  int32_t *len;       // [n] the full length (also beyond cap); 0: no stage won; -1: the precondition does not hold
  int32_t *dist_win;  // [n] or null
  int32_t cap;
  int32_t from_grids;  // 0: the maps are the engine's planes; 1: Params::init_grids, uint8 [n][H][W]
};

// Params::n_envs maps (the engine's own, or a.from_grids) -> a.moves / a.len / a.dist_win
hipError_t launch_solutions(const Params &p, int lpe, const SolArgs &a, hipStream_t s);

}  // namespace pcgrl

#ifdef PCGRL_KERNEL_TU
#include "../pcgrl_kernels2d.h"
#include "../pcgrl_sokoban.h"

namespace pcgrl {

// One stage of the cascade on the workspace bound to c (node 0 = the root): b2 < 0 -> BFSAgent (engine.py:56-74), else
// AStarAgent with balance b2 / 2 (engine.py:96-119).  Returns true on a win: res_h / res_depth of the winning node and its
// index in win_node; else the best node's (h, depth) and whether the open list ran dry.
template <int NH>
__device__ __attribute__((always_inline)) inline bool sol_stage(SokoCtx &c, const SokoPool &pool, int slot, int b2, int max_iter, int &res_h,
                                                                int &res_depth, bool &exhausted, int &win_node) {
  // a fresh epoch of the stage workspace's visited table (entries of earlier epochs read as empty)
  uint32_t *epoch_word = &pool.epochs[slot * SK_STAGES + c.stage];
  uint32_t ep = 0;
  if (c.lane == 0) ep = (atomicAdd(epoch_word, 1u) + 1u) & 0x7FFFu;
  ep = (uint32_t)__builtin_amdgcn_readfirstlane((int)ep);
  if (ep == 0) {  // wrapped: start over with a clean table
    for (int i = c.lane; i < SK_VCAP; i += 64) c.vis[i] = sk_u32x4{0u, 0u, 0u, 0u};
    if (c.lane == 0) ep = (atomicAdd(epoch_word, 1u) + 1u) & 0x7FFFu;
    ep = (uint32_t)__builtin_amdgcn_readfirstlane((int)ep);
  }
  c.epoch = ep;
  c.n_nodes = 1;
  const int DX[4] = {-1, 1, 0, 0}, DY[4] = {0, 0, -1, 1};  // engine.py:3
  int head = 0, tail = 1, best = -1, best_h = 0, best_depth = 0, iters = 0;
  const int h_root = sk_u(SokoNode::unpack(c.nodes[0]).h);
  if (b2 < 0) {
    if (c.lane == 0) c.q[0] = 0u;
  } else {
    sk_hq_store<false>(c, 0, (uint32_t)(2 * h_root) << 16, c.lane == 0);
  }
  while (iters < max_iter && head < tail) {
    iters++;
    head = sk_u(head);
    tail = sk_u(tail);
    c.n_nodes = sk_u(c.n_nodes);
    int cur;
    if (b2 < 0) {  // queue.pop(0)
      cur = sk_u((int)c.q[head]);
      head++;
    } else {  // heapq.heappop
      uint32_t new_top = 0;
      cur = (int)(sk_heappop(c, tail, &new_top) & 0xFFFFu);
    }
    SokoNode nd = SokoNode::unpack(c.nodes[cur]);
    SkCrates<NH> cr;
    cr.load(c, cur);
    nd.depth = sk_u(nd.depth);
    nd.h = sk_u(nd.h);
    nd.px = sk_u(nd.px);
    nd.py = sk_u(nd.py);
    const int px = nd.px, py = nd.py;
    if (c.lv->ntg == c.ncr && c.ncr > 0 && cr.count_on(c.lv->tgt) == c.ncr) {  // checkWin engine.py:272-280
      res_h = nd.h;
      res_depth = nd.depth;
      win_node = cur;
      return true;
    }
    const SkKey key = sk_key(c, px, py, cr);
    if (sk_visited_test_and_set(c, cur, key, cr)) continue;
    if (best < 0 || nd.h < best_h || (nd.h == best_h && nd.depth < best_depth)) {  // engine.py:66-69
      best = cur;
      best_h = nd.h;
      best_depth = nd.depth;
    }
    const int n_dead = cr.count_on(c.lv->dead);
    // Node.getChildren engine.py:14-25 + State.update :298-328
    for (int d = 0; d < 4; d++) {
      const int nx = px + DX[d], ny = py + DY[d];
      if (nx < 0 || ny < 0 || nx > c.lv->w - 1 || ny > c.lv->h - 1 || sk_bit(c.lv->solid, nx, ny)) continue;
      const int moved = cr.at(nx, ny);
      SkCrates<NH> ch = cr;
      int h = nd.h;  // the heuristic depends on the crates only
      if (moved >= 0) {
        const int bx = nx + DX[d], by = ny + DY[d];
        if (!sk_free_cell(c, cr, bx, by)) continue;
        // engine.py:22-23 checkDeadlock over all crates of the child
        const int ndead = n_dead - (sk_bit(c.lv->dead, nx, ny) ? 1 : 0) + (sk_bit(c.lv->dead, bx, by) ? 1 : 0);
        if (ndead > 0) continue;
        ch.move(c, moved, (uint32_t)bx | ((uint32_t)by << 8));
        h = sk_heuristic(c, ch);
      }
      if (c.n_nodes >= c.max_nodes) {  // cannot happen (<= 1 + 4 * iterations nodes per stage); reported if it does
        c.pool_full = true;
        continue;
      }
      const int k = c.n_nodes++;
      ch.store(c, k);
      if (c.lane == 0) {
        SokoNode nn;
        nn.parent = cur;
        nn.depth = nd.depth + 1;
        nn.h = h;
        nn.px = nx;
        nn.py = ny;
        c.nodes[k] = nn.pack();
      }
      if (b2 < 0) {
        if (c.lane == 0) c.q[tail] = (uint32_t)k;
        tail++;
      } else {
        sk_heappush(c, tail, ((uint32_t)(2 * h + b2 * (nd.depth + 1)) << 16) | (uint32_t)k);
      }
    }
  }
  res_h = best_h;
  res_depth = best_depth;
  exhausted = head >= tail;  // the open list ran dry: every reachable state was expanded
  return false;
}

// The reference's cascade (sokoban_prob.py:99-148) on stage workspace 0 of `slot`; sk_cascade's order and shortcut.
template <int NH>
__device__ __attribute__((always_inline)) inline bool sol_cascade(SokoCtx &c, const SokoPool &pool, int slot, int power, int px, int py, int &h,
                                                                  int &depth, int &win_node) {
  sk_bind_at(c, pool, pool.base + (size_t)slot * SK_STAGES * pool.stage_bytes, 0);
  SkCrates<NH> root;  // node 0 = the level's root state
  root.load_level(c, c.lv->root);
  root.store(c, 0);
  const int h0 = sk_heuristic(c, root);
  if (c.lane == 0) {
    SokoNode n0;
    n0.parent = -1;
    n0.depth = 0;
    n0.h = h0;
    n0.px = px;
    n0.py = py;
    c.nodes[0] = n0.pack();
  }
  bool exhausted = false, won = false;
  for (int st = 0; st < SK_STAGES && !won && !exhausted; st++) {  // (one call site: the stage is inlined once)
    bool ex = false;
    won = sol_stage<NH>(c, pool, slot, st == 0 ? -1 : 3 - st, power, h, depth, ex, win_node);
    exhausted = st == 0 && ex;  // (only the BFS stage's flag ends the cascade)
  }
  return won;
}

// Node.getActions of `node` (depth levels below the root) into dst[0 .. min(depth, cap)): every lane follows the parent
// chain (the loads are broadcasts), lane 0 stores.
__device__ inline void sol_walk_back(const SokoCtx &c, int node, int depth, int8_t *dst, int cap, int lane) {
  SokoNode nd = SokoNode::unpack(c.nodes[node]);
  for (int i = depth - 1; i >= 0; i--) {
    const int par = sk_u(nd.parent);
    if (par < 0 || par >= c.max_nodes) break;  // (cannot happen: a node of depth d has d ancestors)
    const SokoNode pn = SokoNode::unpack(c.nodes[par]);
    const int dx = sk_u(nd.px) - sk_u(pn.px), dy = sk_u(nd.py) - sk_u(pn.py);
    const int move = dx < 0 ? 0 : (dx > 0 ? 1 : (dy < 0 ? 2 : 3));
    if (i < cap && lane == 0) dst[i] = (int8_t)move;
    nd = pn;
  }
}

// dst[from .. cap) = -1: bytes up to the first aligned dword, dwords, bytes again
__device__ inline void sol_fill(int8_t *dst, int from, int cap, int lane) {
  if (from >= cap) return;
  uint8_t *b = (uint8_t *)dst + from, *e = (uint8_t *)dst + cap;
  const int headb = (int)((4u - ((uintptr_t)b & 3u)) & 3u);
  uint8_t *a = b + headb < e ? b + headb : e;  // first aligned byte (or the end)
  if (lane < (int)(a - b)) b[lane] = 0xFFu;
  const int nd = (int)((e - a) >> 2);
  uint32_t *w = (uint32_t *)a;
  for (int i = lane; i < nd; i += 64) w[i] = 0xFFFFFFFFu;
  uint8_t *t = a + 4 * (size_t)nd;
  if (lane < (int)(e - t)) t[lane] = 0xFFu;
}

template <int LPE, typename M, bool GRIDS>
__global__ __launch_bounds__(64) void solutions_kernel(Params p, SolArgs a) {
  constexpr int NB = ProbTraits<PCGRL_PROB_SOKOBAN>::NB;
  constexpr bool HUGE = LPE > 8;  // (8 lanes: at most 8 x 32 = 256 cells, 127 pairs)
  constexpr int MAXC = HUGE ? SK_MAXC_HUGE : SK_MAXC;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];  // the top of the A* open list
  Grp<LPE> g;
  g.init();
  const SokoPool &pool = *(const SokoPool *)p.soko;
  const int H = p.cfg.dims[0], W = p.cfg.dims[1];
  const int env = (int)blockIdx.x;  // (the grid is n maps exactly)
  const bool active = g.lane < LPE;  // the map lives in the first lane group
  const bool rowok = active && g.row < H;
  const M colmask = rowok ? (W >= (int)(8 * sizeof(M)) ? ~M(0) : ((M(1) << W) - M(1))) : M(0);
  M b[NB];
  if constexpr (GRIDS) {  // caller bytes, as stats_for_grids_kernel reads them
#pragma unroll
    for (int k = 0; k < NB; k++) b[k] = 0;
    if (rowok) {
      const uint8_t *src = p.init_grids + ((size_t)env * H + g.row) * W;
      for (int x = 0; x < W; x++) {
        const int t = src[x];
#pragma unroll
        for (int k = 0; k < NB; k++) b[k] |= (M)((t >> k) & 1) << x;
      }
    }
  } else {
    load_planes<NB, M>(p, env, g.row, rowok, b);
  }
  // sokoban_prob.py:160-180.  ids: 0 empty 1 solid 2 player 3 crate 4 target (compute_stats' masks and counts)
  const M solid = b[0] & ~b[1] & ~b[2] & colmask, player = ~b[0] & b[1] & ~b[2] & colmask;
  const M crate = b[0] & b[1] & ~b[2] & colmask, target = ~b[0] & ~b[1] & b[2] & colmask;
  const uint32_t c01 = g.gsum((uint32_t)popc_m(player) | ((uint32_t)popc_m(crate) << 16));
  const int n_player = (int)(c01 & 0xFFFFu), n_crate = (int)(c01 >> 16), n_target = (int)g.gsum((uint32_t)popc_m(target));
  const int regions = count_regions(g, (M)(colmask & ~solid));
  const bool need = __builtin_amdgcn_readfirstlane((int)(n_player == 1 && n_crate == n_target && n_crate > 0 && regions == 1)) != 0;
  int dist_win = H * W * (H + W), len = -1;
  int8_t *dst = a.moves + (size_t)env * (size_t)a.cap;
  if (need) {
    len = 0;
    SokoCtx c;
    c.lv = &sk_shared().level;
    c.lane = g.lane;
    c.pool_full = false;
    c.hl = (uint32_t SK_LDS *)(uint32_t *)lds;
    c.hcap = SK_LDS_HEAP;
    c.dbg = nullptr;
    // take a workspace slot (lane 0; the slot index is broadcast) -- sokoban_solve's protocol
    int slot = 0;
    if (g.lane == 0) {
      int s = (int)((blockIdx.x * 7u) % (unsigned)pool.n_slots);
      while (atomicCAS(&pool.locks[s], 0, 1) != 0) {
        s = (s + 1) % pool.n_slots;
        __builtin_amdgcn_s_sleep(8);
      }
      slot = s;
    }
    slot = __builtin_amdgcn_readfirstlane(slot);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    int px = 0, py = 0, ncr = 0, ntg = 0;
    sk_build_level<LPE, M, MAXC>(g, 0, H, W, solid, player, crate, target, px, py, ncr, ntg);
    if (ncr > MAXC || ntg > MAXC || W + 2 > SK_MAXDIM || H + 2 > SK_MAXDIM) {
      if (g.lane == 0) atomicOr(p.err, 2);  // beyond the device solver's limits: reported by pcgrl_poll_error
    } else {
      c.ncr = ncr;
      c.cstride = (ncr + 3) & ~3;
      if (g.lane == 0) {
        sk_shared().level.ncr = ncr;
        sk_shared().level.ntg = ntg;
      }
      sk_init_deadlocks(c);
      bool won = false;
      int h = 0, depth = 0, win_node = 0;
      // the register forms of sokoban_solve: a map's solution and its sol-length come from the same search
      if (ncr > SK_MAXC) {
        if constexpr (HUGE) won = sol_cascade<SK_NH_HUGE>(c, pool, slot, p.cfg.solver_power, px, py, h, depth, win_node);
      } else if (ncr > 64) {
        won = sol_cascade<2>(c, pool, slot, p.cfg.solver_power, px, py, h, depth, win_node);
      } else {
        won = sol_cascade<1>(c, pool, slot, p.cfg.solver_power, px, py, h, depth, win_node);
      }
      if (won) {
        dist_win = 0;
        len = depth;
        sol_walk_back(c, win_node, depth, dst, a.cap, g.lane);
      } else {
        dist_win = h;  // heuristic of the last stage's best node (sokoban_prob.py:147)
      }
      if (c.pool_full && g.lane == 0) atomicOr(p.err, 2);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (g.lane == 0) atomicExch(&pool.locks[slot], 0);
  }
  sol_fill(dst, len > 0 ? len : 0, a.cap, g.lane);
  if (g.lane == 0) {
    a.len[env] = len;
    if (a.dist_win != nullptr) a.dist_win[env] = dist_win;
  }
}

template <int LPE, typename M>
static hipError_t launch_solutions_pl(const Params &p, const SolArgs &a, hipStream_t s) {
  const dim3 grid(p.n_envs), block(64);
  const size_t lds = (size_t)SK_LDS_HEAP * sizeof(uint32_t);
  if (a.from_grids)
    hipLaunchKernelGGL((solutions_kernel<LPE, M, true>), grid, block, lds, s, p, a);
  else
    hipLaunchKernelGGL((solutions_kernel<LPE, M, false>), grid, block, lds, s, p, a);
  return hipGetLastError();
}

}  // namespace pcgrl
#endif
