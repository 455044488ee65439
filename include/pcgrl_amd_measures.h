/*
 * pcgrl_amd_measures.h -- level measures and pairwise Hamming diversity of libpcgrl_amd.so (companion of pcgrl_amd.h).
 *
 * What a quality-diversity or evaluation loop needs per generation beside the statistics: the behaviour characteristics that
 * place a level in the archive (evo/evolve.py:606-635 get_bc -> :423-592 get_entropy, get_counts, get_emptiness,
 * get_hor_sym, get_ver_sym, get_sym, get_co) and the diversity of a set of levels (rl/evaluate_ctrl.py:42-48 div_calc;
 * evo/evolve.py:1236-1244 diversity_bonus).  The kernels hand out the INTEGERS behind them and, beside them, the float64
 * forms: one or two correctly rounded double operations on these integers in the reference's order (the library is built
 * without fast-math and without contraction), so they equal numpy's bit for bit (n = H * W, T tile types):
 *
 *   d_counts[e][t]   cells of map e with tile t        get_counts = counts / n; emptiness = counts[0] / n
 *   d_match[e][0]    horizontal matches: cells of the top H / 2 rows equal to their mirror cell in the bottom H / 2 rows
 *                    (the middle row of an odd H is left out)     symmetry-horizontal = match / (W * H / 2)
 *   d_match[e][1]    vertical matches, the same over the left W / 2 columns   symmetry-vertical = match / (W * H / 2)
 *                    -- W * H / 2 is a float division: a perfectly symmetric 7 x 11 map scores below 1;
 *                    symmetry = (vertical + horizontal) / 2.0
 *   d_match[e][2]    co-occurance: equal np.roll neighbours summed over the four directions and all cells; the rolls wrap
 *                    around (H == 1: a cell is its own vertical neighbour; H == 2: both vertical rolls meet the same cell)
 *                    co-occurance = match / (4 * n)
 *   d_forms[e][..]   double [n][5 + T]: emptiness, symmetry-horizontal, symmetry-vertical, symmetry, co-occurance as above, then
 *                    get_counts' T fractions
 *   d_entropy[e]     get_entropy itself, in double on the device: e = 0.0; for t = 0 .. T - 1: if counts[t] != 0:
 *                    e -= tab[counts[t]]; e / tab[n + 1].  d_entropy_tab is the caller's table of n + 2 doubles,
 *                    tab[c] = (c / n) * ln(c / n) for c = 0 .. n (tab[0] is never read) and tab[n + 1] =
 *                    -(1 / T) * ln(1 / T) * T: built with the logarithm the caller wants reproduced (numpy's, to equal
 *                    get_entropy bit for bit on that host).
 *   Hamming distance d(a, b) = cells whose tiles differ (one cell counts once).  `group` = K cuts the n maps into n / K
 *   consecutive groups:
 *   d_sum[g]         S = sum of d over all ordered pairs of group g (int64)
 *   d_scores[g][2]   double: div_calc = S / (K * (K - 1)) / n;  diversity_bonus = 10 * (S / (K * K - 1)) / n
 *   d_nearest[i]     min over k != i of the same group of d(i, k);  d_nearest_idx[i]: that k as an index within the group, the
 *                    LOWEST on ties
 *   d_pairwise       int32 [n / K][K][K]: the symmetric matrix with its zero diagonal
 *
 * 2-D problems only (binary, zelda, sokoban; every supported map shape).  The 3-D maze is PCGRL_EUNSUPPORTED: the
 * reference's get_counts reads an attribute that does not exist there and get_co looks at two axes only.
 *
 * The measures are functions of the maps alone (stale statistics after pcgrl_update do not matter).  Caller maps are uint8
 * [n][H][W] tile ids; ids are masked to the ceil(log2 T) bits the engine keeps of a tile (as pcgrl_stats_for_grids_h reads
 * its inputs), so an id >= T of binary / zelda aliases a tile and a sokoban id 5..7 matches no count but still compares.
 * Every entry point only enqueues kernels on `stream` (HIP-graph capturable; no allocation: the caller supplies the
 * scratch), checks its handle, pointers, n >= 0 and group (PCGRL_EINVAL) and the problem (PCGRL_EUNSUPPORTED) before any HIP
 * call, runs on the engine's device and restores the caller's.  n == 0 is a no-op.  All pointers are device pointers.
 */
#ifndef PCGRL_AMD_MEASURES_H
#define PCGRL_AMD_MEASURES_H
#include <stddef.h>

#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* T, the tile types of h's problem (the row length of d_counts); 0 for the 3-D maze; -1 on a null handle */
int32_t pcgrl_measures_tiles(pcgrl_handle h);

/* The measures of the CURRENT map of every env of h (n = the engine's batch).  d_counts int32 [n][T] and d_match int32
 * [n][3] are required; d_forms double [n][5 + T] and d_entropy double [n] may each be NULL, and only with d_entropy is
 * d_entropy_tab read. */
int pcgrl_measures(pcgrl_handle h, int32_t *d_counts, int32_t *d_match, double *d_forms, double *d_entropy,
                   const double *d_entropy_tab, void *stream);

/* The same for n caller maps; n is independent of the engine's batch. */
int pcgrl_measures_for_grids(pcgrl_handle h, int32_t n, const uint8_t *d_grids, int32_t *d_counts, int32_t *d_match,
                             double *d_forms, double *d_entropy, const double *d_entropy_tab, void *stream);

/* bytes of the scratch pcgrl_diversity* need for n maps (their bit-plane image and one nearest-map key each:
 * 8 * (ceil(log2 T) * ceil(H * W / 64) + 1) per map);
 * 0 for an unsupported problem, a null handle or n <= 0 */
size_t pcgrl_diversity_scratch_bytes(pcgrl_handle h, int32_t n);

/* Pairwise Hamming distances among the CURRENT maps of h, in consecutive groups of `group` maps (group >= 2 and a divisor of
 * the batch, else PCGRL_EINVAL).  d_scratch (8-byte aligned) and d_sum int64 [n / group] are required; d_scores double
 * [n / group][2], d_nearest, d_nearest_idx int32 [n] and d_pairwise may each be NULL. */
int pcgrl_diversity(pcgrl_handle h, int32_t group, void *d_scratch, int64_t *d_sum, double *d_scores, int32_t *d_nearest,
                    int32_t *d_nearest_idx, int32_t *d_pairwise, void *stream);

/* The same for n caller maps. */
int pcgrl_diversity_for_grids(pcgrl_handle h, int32_t n, const uint8_t *d_grids, int32_t group, void *d_scratch, int64_t *d_sum,
                              double *d_scores, int32_t *d_nearest, int32_t *d_nearest_idx, int32_t *d_pairwise, void *stream);

#ifdef __cplusplus
}
#endif
#endif
