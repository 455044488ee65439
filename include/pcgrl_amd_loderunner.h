/*
 * pcgrl_amd_loderunner.h -- Lode Runner levels of libpcgrl_amd.so (companion of pcgrl_amd.h).
 *
 * One launch evaluates n Lode Runner levels: what LoderunnerProblem.get_stats returns for each
 * (envs/probs/loderunner_prob.py:78-91 -- three tile counts and, with exactly one player, the gold searches of
 * envs/probs/loderunner/engine.py:get_score), the loss ControlWrapper.get_loss would derive from it, and the per-gold record
 * behind `win` and `path-length`.  A map is uint8 [H][W] of tile ids
 *
 *   0 empty   1 brick   2 ladder   3 rope   4 solid   5 gold   6 enemy   7 player       (loderunner_prob.py:46)
 *
 * and the statistics come in get_stats' order:
 *
 *   0 player   1 enemies   2 gold   3 win   4 path-length
 *
 * The reference abandons an evaluation after one second of wall clock (engine.py:254, 287, 293).  The device has no such
 * limit: its result is the reference's with the clock stopped.  At the stock 8 x 12 the reference's limit does not bite;
 * above it the reference's own answer depends on the host's speed.
 *
 * Stepping Lode Runner environments is not part of the engine: pcgrl_create still refuses the problem, and nothing here
 * needs a pcgrl_handle.
 *
 * pcgrl_loderunner_evaluate checks its arguments before any HIP call -- PCGRL_EINVAL: null cfg, grids or stats, n < 1,
 * gold_cap < 0, a workspace that is null, not 4-byte aligned or smaller than pcgrl_loderunner_workspace_bytes;
 * PCGRL_EUNSUPPORTED: a shape outside 1..16 x 1..32 -- and then only enqueues one kernel on `stream` of the current device:
 * no allocation, no synchronisation, HIP-graph capturable.  The kernel initialises everything it reads of the workspace, so
 * what an earlier call left there does not matter; two calls that may run at the same time need a workspace each.
 *
 * Outputs (device pointers; every one but d_stats may be NULL):
 *   d_stats       double [n][5]: every value exactly the double of the reference's Python value; win is one correctly
 *                 rounded division 1 / (1 + (golds - collected)), -1 without gold, 0 when player != 1
 *   d_loss        double [n]: sum over the statistics with has_trg of -(distance of the value to [trg_lo, trg_hi]) * weight,
 *                 in order, each term one multiplication and one addition in double
 *   d_play        int32 [n][4]: searched (player == 1), landing row, landing column (-1, -1 when not searched), golds
 *                 collected including those on the starting fall
 *   d_gold_state  int8 [n][gold_cap]: per gold in row-major order 0 not collected, 1 by its own pair of searches, 2 on
 *                 another gold's path, 3 on the starting fall; -1 past the last gold
 *   d_gold_dist   int16 [n][gold_cap]: what that gold added to path-length; 0 unless the state is 1
 *   d_error       uint32 [n]: bit 0 = a tile id above 7 was read as empty
 * path-length and the collected count stay complete when gold_cap is smaller than the number of golds.
 */
#ifndef PCGRL_AMD_LODERUNNER_H
#define PCGRL_AMD_LODERUNNER_H
#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCGRL_LODERUNNER_STATS 5

typedef struct pcgrl_loderunner_config {
  int32_t h, w; /* 1..16 x 1..32 */
  int32_t has_trg[PCGRL_LODERUNNER_STATS];
  double weight[PCGRL_LODERUNNER_STATS];
  double trg_lo[PCGRL_LODERUNNER_STATS], trg_hi[PCGRL_LODERUNNER_STATS]; /* the zero-loss interval, both ends included */
} pcgrl_loderunner_config;

/* bytes of workspace a launch over n levels needs: one slot per block, per slot 64 searches of 4 h w + 1 nodes,
 * h + w + h w + 1 buckets and h w cells of 4 bytes; min(n, B) blocks, B = as many slots as fit 640 MiB, at least 256 and at
 * most 4096 (4096 at 8 x 12, 839 at 16 x 32); -1 for arguments pcgrl_loderunner_evaluate would refuse */
int64_t pcgrl_loderunner_workspace_bytes(int32_t n, int32_t h, int32_t w);

int pcgrl_loderunner_evaluate(const pcgrl_loderunner_config *cfg, int32_t n, const uint8_t *d_grids, void *d_workspace,
                              int64_t workspace_bytes, int32_t gold_cap, double *d_stats, double *d_loss, int32_t *d_play,
                              int8_t *d_gold_state, int16_t *d_gold_dist, uint32_t *d_error, void *stream);

#ifdef __cplusplus
}
#endif
#endif
