/*
 * pcgrl_amd_ddave.h -- Dangerous Dave levels of libpcgrl_amd.so (companion of pcgrl_amd.h).
 *
 * One launch evaluates n Dangerous Dave levels: what DDaveProblem.get_stats returns for each
 * (envs/probs/ddave/ddave_prob.py:149-169) -- seven map statistics and, for a level with one player, one exit, one key and one
 * region, the play-through of ddave/engine.py: up to four searches (A* at balance 1, 0.5 and 0, then BFS) of at most
 * solver_power iterations each.  A map is uint8 [H][W] of tile ids
 *
 *   0 empty   1 solid   2 player   3 exit   4 diamond   5 key   6 spike            (ddave_prob.py:53-54)
 *
 * and the statistics come in get_stats' order, as int32:
 *
 *   0 player   1 dist-floor   2 exit   3 diamonds   4 key   5 spikes   6 regions   7 num-jumps   8 col-diamonds
 *   9 dist-win   10 sol-length
 *
 * dist-floor sums, over the player tiles, dy - 1 of the first solid tile below (H - 1 without one; no border).  regions counts
 * the 4-connected components of every tile but solid and spike.  Without a play-through dist-win is W * H and the three play
 * statistics are 0.  The play-through runs on the level with a solid border, (H + 2) x (W + 2); its heuristic is the Manhattan
 * distance to the door, or to the key plus (W + 2) + (H + 2) while the key lies on the map, minus 5 per collected diamond, so
 * dist-win can be negative.  The first stage that wins ends the chain: dist-win 0, sol-length the winner's depth; when none
 * wins, dist-win is the heuristic of the BFS's best node and sol-length 0; num-jumps and col-diamonds are the returned node's.
 * The open list of the A* stages is CPython's heapq ordered by heuristic + balance * depth with `<` alone; the visited key is
 * (x, y, key on the map, remaining diamonds).  DESIGN.md section 31 has every rule.
 *
 * The remaining diamonds are a 64-bit set: a level that reaches the play-through with more than 64 diamonds is not searched.
 * It reports the statistics of a level without a play-through and play status 5; no error bit is set.
 *
 * Stepping Dangerous Dave environments is not part of the engine: pcgrl_create does not know the problem, and nothing here
 * needs a pcgrl_handle.
 *
 * pcgrl_ddave_evaluate checks its arguments before any HIP call -- PCGRL_EINVAL: null cfg, grids or stats, n < 1, move_cap < 0,
 * a workspace that is null, not 16-byte aligned or smaller than pcgrl_ddave_workspace_bytes; PCGRL_EUNSUPPORTED: a shape outside
 * 1..16 x 1..32 or a solver_power outside 1..16000 -- and then only enqueues one kernel on `stream` of the current device: no
 * allocation, no synchronisation, HIP-graph capturable.  d_grids may have any alignment.  The workspace need not be cleared.
 *
 * Outputs (device pointers; every one but d_stats may be NULL, and a NULL output is neither computed nor written):
 *   d_stats   int32 [n][11]
 *   d_moves   int8 [n][move_cap]: the returned node's actions from the start (0 stay, 1 left, 2 right, 3 jump), -1 past the
 *             end; all -1 without a play-through.  Ignored when move_cap is 0.
 *   d_length  int32 [n]: the number of actions, whatever move_cap cuts
 *   d_play    int32 [n][12]: 0 status (-1 not searched, 0 no stage won, 1..4 the stage that won, 5 too many diamonds);
 *             1..4 the iterations of each stage (0 for a stage not run); 5, 6 the returned node's x, y in bordered coordinates;
 *             7 airTime; 8 health; 9 col_key; 10 the diamonds in the level; 11 the returned node's depth.  5..9 and 11 are 0
 *             without a play-through.
 *   d_error   uint32 [n]: bit 0 = a tile id above 6 was read as solid
 *
 * The measures and the pairwise Hamming diversity of such maps: the quantities, the rules and the order of the double
 * operations are those of pcgrl_amd_measures.h -- read that header for d_counts, d_match, d_forms, d_entropy / d_entropy_tab,
 * d_sum, d_scores, d_nearest, d_nearest_idx and d_pairwise -- with T = 7 tile types (d_counts is int32 [n][7], d_forms double
 * [n][12]) and n_cells = h * w; tile ids are masked to 3 bits (7 counts nowhere) and set no error.  The argument lists and the
 * checks are those of pcgrl_amd_microstructure.h, with this header's shape range.
 */
#ifndef PCGRL_AMD_DDAVE_H
#define PCGRL_AMD_DDAVE_H
#include <stddef.h>

#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCGRL_DDAVE_STATS 11
#define PCGRL_DDAVE_WEIGHTS 10
#define PCGRL_DDAVE_PLAY 12

typedef struct pcgrl_ddave_config {
  int32_t h, w;         /* 1..16 x 1..32 */
  int32_t solver_power; /* 1..16000: the iterations of each of the four searches */
  /* the reward's bounds and the episode's targets (ddave_prob.py:23-29): the kernel does not read them */
  int32_t max_diamonds, min_spikes, target_jumps, target_solution;
  /* the reward's weights in its order of summation (ddave_prob.py:196-205): player, dist-floor, exit, spikes, diamonds, key,
   * regions, num-jumps, dist-win, sol-length */
  double weight[PCGRL_DDAVE_WEIGHTS];
} pcgrl_ddave_config;

/* bytes of the search workspace for n levels (per level 20 * (4 * power + 1) for the nodes and the open list, rounded up to 16,
 * and 12 * C for the visited set, C the power of two with 2 * power <= C, at least 16); negative outside the limits or n < 1 */
int64_t pcgrl_ddave_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t solver_power);

int pcgrl_ddave_evaluate(const pcgrl_ddave_config *cfg, int32_t n, const uint8_t *d_grids, void *d_workspace,
                         int64_t workspace_bytes, int32_t move_cap, int32_t *d_stats, int8_t *d_moves, int32_t *d_length,
                         int32_t *d_play, uint32_t *d_error, void *stream);

/* The measures of n caller maps.  d_counts int32 [n][7] and d_match int32 [n][3] are required; d_forms double [n][12] and
 * d_entropy double [n] may each be NULL, and only with d_entropy is d_entropy_tab (h * w + 2 doubles, T = 7) read. */
int pcgrl_ddave_measures_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t *d_counts, int32_t *d_match,
                                   double *d_forms, double *d_entropy, const double *d_entropy_tab, void *stream);

/* bytes of the scratch the diversity call needs for n maps of h x w (their bit-plane image and one nearest-map key each:
 * 8 * (3 * ceil(h * w / 64) + 1) per map); 0 for an unsupported shape or n <= 0 */
size_t pcgrl_ddave_diversity_scratch_bytes(int32_t h, int32_t w, int32_t n);

/* Pairwise Hamming distances among n caller maps in consecutive groups of `group` maps.  d_scratch (8-byte aligned) and d_sum
 * int64 [n / group] are required; d_scores double [n / group][2], d_nearest, d_nearest_idx int32 [n] and d_pairwise int32
 * [n / group][group][group] may each be NULL. */
int pcgrl_ddave_diversity_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t group, void *d_scratch,
                                    int64_t *d_sum, double *d_scores, int32_t *d_nearest, int32_t *d_nearest_idx,
                                    int32_t *d_pairwise, void *stream);

#ifdef __cplusplus
}
#endif
#endif
