/*
 * pcgrl_amd_mdungeon.h -- MiniDungeon levels of libpcgrl_amd.so (companion of pcgrl_amd.h).
 *
 * One launch evaluates n MiniDungeon levels: what MDungeonProblem.get_stats returns for each
 * (envs/probs/mdungeon/mdungeon_prob.py:151-171) -- six map statistics and, for a level with one player, one exit and one
 * region, the play-through of mdungeon/engine.py: up to four searches (A* at balance 1, 0.5 and 0, then BFS) of at most
 * solver_power iterations each.  A map is uint8 [H][W] of tile ids
 *
 *   0 empty   1 solid   2 player   3 exit   4 potion   5 treasure   6 goblin   7 ogre      (mdungeon_prob.py:50-51)
 *
 * and the statistics come in get_stats' order, as int32:
 *
 *   0 player   1 exit   2 potions   3 treasures   4 enemies   5 regions   6 col-potions   7 col-treasures   8 col-enemies
 *   9 dist-win   10 sol-length
 *
 * enemies counts goblins and ogres together.  regions counts the 4-connected components of every tile but solid.  Without a
 * play-through dist-win is W * H and the four play statistics are 0.  The play-through runs on the level with a solid border,
 * (H + 2) x (W + 2); the player starts at health 5 and moves left, right, up or down (a move into a solid cell changes
 * nothing); a potion gives 2 health up to 5, a goblin costs 1 and an ogre 2 down to 0, each item once; health 0 loses and the
 * door wins.  The heuristic is the Manhattan distance to the door plus 4 * (5 - health) minus 4 per collected treasure, so
 * dist-win can be negative.  The first stage that wins ends the chain: dist-win 0, sol-length the winner's depth; when none
 * wins, dist-win is the heuristic of the BFS's best node and sol-length 0; the three col-* statistics are the returned node's.
 * The open list of the A* stages is CPython's heapq ordered by heuristic + balance * depth with `<` alone; the visited key is
 * (x, y, health, remaining items).  DESIGN.md section 32 has every rule.
 *
 * The remaining potions, treasures and enemies are one 64-bit set, indexed by the item cell's row-major ordinal: a level that
 * reaches the play-through with more than 64 items is not searched.  It reports the statistics of a level without a
 * play-through and play status 5; no error bit is set.
 *
 * The open list's order is kept as the 16-bit integer 2 * heuristic + (2 * balance) * depth + 512: the heuristic is at least
 * -4 * 64, hence the bias of 2 * 4 * 64, and at most 50 + 20 with a depth below 16 000, hence 2 * 70 + 32 000 + 512 < 65 536.
 *
 * Stepping MiniDungeon environments is not part of the engine: pcgrl_create does not know the problem, and nothing here needs
 * a pcgrl_handle.
 *
 * pcgrl_mdungeon_evaluate checks its arguments before any HIP call -- PCGRL_EINVAL: null cfg, grids or stats, n < 1,
 * move_cap < 0, a workspace that is null, not 16-byte aligned or smaller than pcgrl_mdungeon_workspace_bytes;
 * PCGRL_EUNSUPPORTED: a shape outside 1..16 x 1..32 or a solver_power outside 1..16000 -- and then only enqueues one kernel on
 * `stream` of the current device: no allocation, no synchronisation, HIP-graph capturable.  d_grids may have any alignment.
 * The workspace need not be cleared.
 *
 * Outputs (device pointers; every one but d_stats may be NULL, and a NULL output is neither computed nor written):
 *   d_stats   int32 [n][11]
 *   d_moves   int8 [n][move_cap]: the returned node's actions from the start (0 left, 1 right, 2 up, 3 down), -1 past the end;
 *             all -1 without a play-through.  Ignored when move_cap is 0.
 *   d_length  int32 [n]: the number of actions, whatever move_cap cuts
 *   d_play    int32 [n][12]: 0 status (-1 not searched, 0 no stage won, 1..4 the stage that won, 5 too many items); 1..4 the
 *             iterations of each stage (0 for a stage not run); 5, 6 the returned node's x, y in bordered coordinates;
 *             7 health; 8 col_potions; 9 col_treasures; 10 col_enemies; 11 the returned node's depth.  1..11 are 0 without a
 *             play-through.
 *   d_error   uint32 [n]: bit 0 = a tile id above 7 was read as solid
 *
 * The measures and the pairwise Hamming diversity of such maps: the quantities, the rules and the order of the double
 * operations are those of pcgrl_amd_measures.h -- read that header for d_counts, d_match, d_forms, d_entropy / d_entropy_tab,
 * d_sum, d_scores, d_nearest, d_nearest_idx and d_pairwise -- with T = 8 tile types (d_counts is int32 [n][8], d_forms double
 * [n][12]) and n_cells = h * w; tile ids are masked to 3 bits and set no error.  The argument lists and the checks are those of
 * pcgrl_amd_microstructure.h, with this header's shape range.
 */
#ifndef PCGRL_AMD_MDUNGEON_H
#define PCGRL_AMD_MDUNGEON_H
#include <stddef.h>

#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCGRL_MDUNGEON_STATS 11
#define PCGRL_MDUNGEON_WEIGHTS 9
#define PCGRL_MDUNGEON_PLAY 12

typedef struct pcgrl_mdungeon_config {
  int32_t h, w;         /* 1..16 x 1..32 */
  int32_t solver_power; /* 1..16000: the iterations of each of the four searches */
  /* the reward's bounds and the episode's targets (mdungeon_prob.py:25-30): the kernel does not read them */
  int32_t max_enemies, max_potions, max_treasures, target_solution;
  double target_col_enemies;
  /* the reward's weights in its order of summation (mdungeon_prob.py:197-205): player, exit, enemies, treasures, potions,
   * regions, col-enemies, dist-win, sol-length */
  double weight[PCGRL_MDUNGEON_WEIGHTS];
} pcgrl_mdungeon_config;

/* bytes of the search workspace for n levels (per level 20 * (4 * power + 1) for the nodes and the open list, rounded up to 16,
 * and 12 * C for the visited set, C the power of two with 2 * power <= C, at least 16); negative outside the limits or n < 1 */
int64_t pcgrl_mdungeon_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t solver_power);

int pcgrl_mdungeon_evaluate(const pcgrl_mdungeon_config *cfg, int32_t n, const uint8_t *d_grids, void *d_workspace,
                            int64_t workspace_bytes, int32_t move_cap, int32_t *d_stats, int8_t *d_moves, int32_t *d_length,
                            int32_t *d_play, uint32_t *d_error, void *stream);

/* The measures of n caller maps.  d_counts int32 [n][8] and d_match int32 [n][3] are required; d_forms double [n][12] and
 * d_entropy double [n] may each be NULL, and only with d_entropy is d_entropy_tab (h * w + 2 doubles, T = 8) read. */
int pcgrl_mdungeon_measures_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t *d_counts,
                                      int32_t *d_match, double *d_forms, double *d_entropy, const double *d_entropy_tab,
                                      void *stream);

/* bytes of the scratch the diversity call needs for n maps of h x w (their bit-plane image and one nearest-map key each:
 * 8 * (3 * ceil(h * w / 64) + 1) per map); 0 for an unsupported shape or n <= 0 */
size_t pcgrl_mdungeon_diversity_scratch_bytes(int32_t h, int32_t w, int32_t n);

/* Pairwise Hamming distances among n caller maps in consecutive groups of `group` maps.  d_scratch (8-byte aligned) and d_sum
 * int64 [n / group] are required; d_scores double [n / group][2], d_nearest, d_nearest_idx int32 [n] and d_pairwise int32
 * [n / group][group][group] may each be NULL. */
int pcgrl_mdungeon_diversity_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t group, void *d_scratch,
                                       int64_t *d_sum, double *d_scores, int32_t *d_nearest, int32_t *d_nearest_idx,
                                       int32_t *d_pairwise, void *stream);

#ifdef __cplusplus
}
#endif
#endif
