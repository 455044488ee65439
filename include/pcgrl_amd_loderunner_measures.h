/*
 * pcgrl_amd_loderunner_measures.h -- level measures and pairwise Hamming diversity of Lode Runner maps (companion of
 * pcgrl_amd_loderunner.h).
 *
 * The quantities, the rules and the order of the double operations are those of pcgrl_amd_measures.h -- read that header for
 * d_counts, d_match, d_forms, d_entropy / d_entropy_tab, d_sum, d_scores, d_nearest, d_nearest_idx and d_pairwise -- with
 * T = 8 tile types (pcgrl_amd_loderunner.h's ids 0..7: d_counts is int32 [n][8], d_forms double [n][13]) and n_cells = h * w.
 * The reference computes exactly these on Lode Runner levels: its quality-diversity loop places a level in the archive with
 * get_bc on the integer map (evo/evolve.py:606-635; configs/evo/batch.yaml pairs "emptiness" and "symmetry" with
 * "path-length" for this problem), adds diversity_bonus (evo/evolve.py:1236-1244), and rl/evaluate_ctrl.py:42-48 div_calc
 * scores the final maps of an evaluation run.
 *
 * Shapes: every shape pcgrl_loderunner_evaluate takes, 1..16 rows x 1..32 columns; anything else is PCGRL_EUNSUPPORTED.  What
 * such shapes bring:
 *   h == 1      the np.roll of get_co wraps: a cell is its own vertical neighbour, twice (2 matches per cell), and there are
 *               no horizontal-symmetry pairs (d_match[e][0] == 0)
 *   w == 1      the same along the other axis (d_match[e][1] == 0)
 *   w == 2      both horizontal rolls meet the same cell (h == 2 likewise)
 *   1 x 1       the symmetry divisor w * h / 2 is 0.5 and there are no pairs: symmetry 0; every co-occurance comparison
 *               matches: 1.0
 *   odd h, w    the middle row / column is left out of the symmetry pairs; the divisor w * h / 2 is a float division and need
 *               not be an integer (5 x 7: 17.5), so a perfectly symmetric map scores below 1
 * The divisors are the map's own h * w, not the 12 x 8 the problem's targets are frozen at.
 *
 * Tile ids are masked to 3 bits, as pcgrl_amd_measures.h masks to ceil(log2 T) bits: with T = 8 every masked id is a counted
 * tile, ids >= 8 alias, and no error bit is set anywhere (pcgrl_loderunner_evaluate's own convention, an id above 7 read as
 * empty with bit 0 of d_error, is untouched and differs).
 *
 * The calls take no handle and run on the current device, like pcgrl_loderunner_evaluate; d_grids is uint8 [n][h][w] at any
 * alignment.
 *
 * Every entry point checks its arguments before any HIP call -- PCGRL_EINVAL: a null required pointer, n < 0, d_entropy
 * without d_entropy_tab, a group below 2 or one that does not divide n, a d_scratch that is not 8-byte aligned;
 * PCGRL_EUNSUPPORTED: a shape outside 1..16 x 1..32 -- and then only enqueues kernels on `stream`: no allocation (the caller
 * supplies the scratch), no synchronisation, HIP-graph capturable.  n == 0 is a no-op.  All pointers are device pointers.
 */
#ifndef PCGRL_AMD_LODERUNNER_MEASURES_H
#define PCGRL_AMD_LODERUNNER_MEASURES_H
#include <stddef.h>

#include "pcgrl_amd_loderunner.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The measures of n caller maps.  d_counts int32 [n][8] and d_match int32 [n][3] are required; d_forms double [n][13] and
 * d_entropy double [n] may each be NULL, and only with d_entropy is d_entropy_tab (h * w + 2 doubles, T = 8) read. */
int pcgrl_loderunner_measures_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t *d_counts,
                                        int32_t *d_match, double *d_forms, double *d_entropy, const double *d_entropy_tab,
                                        void *stream);

/* bytes of the scratch the diversity call needs for n maps of h x w (their bit-plane image and one nearest-map key each:
 * 8 * (3 * ceil(h * w / 64) + 1) per map); 0 for an unsupported shape or n <= 0 */
size_t pcgrl_loderunner_diversity_scratch_bytes(int32_t h, int32_t w, int32_t n);

/* Pairwise Hamming distances among n caller maps in consecutive groups of `group` maps.  d_scratch (8-byte aligned) and d_sum
 * int64 [n / group] are required; d_scores double [n / group][2], d_nearest, d_nearest_idx int32 [n] and d_pairwise int32
 * [n / group][group][group] may each be NULL. */
int pcgrl_loderunner_diversity_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t group,
                                         void *d_scratch, int64_t *d_sum, double *d_scores, int32_t *d_nearest,
                                         int32_t *d_nearest_idx, int32_t *d_pairwise, void *stream);

#ifdef __cplusplus
}
#endif
#endif
