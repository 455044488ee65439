/*
 * pcgrl_amd_smb_measures.h -- level measures and pairwise Hamming diversity of Super Mario Bros maps (companion of
 * pcgrl_amd_smb.h and pcgrl_amd_smb_env.h).
 *
 * The quantities, the rules and the order of the double operations are those of pcgrl_amd_measures.h -- read that header for
 * d_counts, d_match, d_forms, d_entropy / d_entropy_tab, d_sum, d_scores, d_nearest, d_nearest_idx and d_pairwise -- with
 * T = 7 tile types (pcgrl_amd_smb.h's ids 0..6: d_counts is int32 [n][7], d_forms double [n][12]) and n_cells = h * w.  The
 * reference computes exactly these on Mario levels: its quality-diversity loop places a level in the archive with get_bc on
 * the integer map (evo/evolve.py:606-635), adds diversity_bonus (evo/evolve.py:1236-1244), and rl/evaluate_ctrl.py:42-48
 * div_calc scores the final maps of an evaluation run.
 *
 * Shapes: every shape the SMB evaluator takes, 4..16 rows x 1..128 columns; anything else is PCGRL_EUNSUPPORTED.  What such
 * shapes bring that the 2-D engine's never did:
 *   w > 64      a row is longer than the 64 cells a wave handles at a time; the results do not depend on it
 *   w == 1      the np.roll of get_co wraps: a cell is its own horizontal neighbour, twice (2 matches per cell), and there are
 *               no vertical-symmetry pairs (d_match[e][1] == 0)
 *   w == 2      both horizontal rolls meet the same cell
 *   odd h, w    the middle row / column is left out of the symmetry pairs; the divisor w * h / 2 is a float division and need
 *               not be an integer (5 x 7: 17.5), so a perfectly symmetric map scores below 1
 *
 * Tile ids are masked to 3 bits, as pcgrl_amd_measures.h masks to ceil(log2 T) bits: id 7 matches no count but still compares,
 * ids >= 8 alias, and no error bit is set anywhere (the evaluator's d_error and the env handle's error word are untouched).
 *
 * The _for_grids calls take no handle and run on the current device, like pcgrl_smb_evaluate; d_grids is uint8 [n][h][w] at
 * any alignment.  The _env_ calls read the committed maps of a pcgrl_smb_env_handle (n = its n_envs) on the handle's device and
 * restore the caller's; under a solver budget (pcgrl_amd_smb_ready.h) a busy env's step in flight is not shown, as in
 * pcgrl_smb_env_get_state.  Enqueue them after the reset / step they are to show, on the same stream.
 *
 * Every entry point checks its arguments before any HIP call -- PCGRL_EINVAL: a null handle or required pointer, n < 0,
 * d_entropy without d_entropy_tab, a group below 2 or one that does not divide n, a d_scratch that is not 8-byte aligned;
 * PCGRL_EUNSUPPORTED: a shape outside 4..16 x 1..128 -- and then only enqueues kernels on `stream`: no allocation (the caller
 * supplies the scratch), no synchronisation, HIP-graph capturable.  n == 0 is a no-op.  All pointers are device pointers.
 */
#ifndef PCGRL_AMD_SMB_MEASURES_H
#define PCGRL_AMD_SMB_MEASURES_H
#include <stddef.h>

#include "pcgrl_amd_smb_env.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The measures of n caller maps.  d_counts int32 [n][7] and d_match int32 [n][3] are required; d_forms double [n][12] and
 * d_entropy double [n] may each be NULL, and only with d_entropy is d_entropy_tab (h * w + 2 doubles, T = 7) read. */
int pcgrl_smb_measures_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t *d_counts, int32_t *d_match,
                                 double *d_forms, double *d_entropy, const double *d_entropy_tab, void *stream);

/* bytes of the scratch the diversity calls need for n maps of h x w (their bit-plane image and one nearest-map key each:
 * 8 * (3 * ceil(h * w / 64) + 1) per map); 0 for an unsupported shape or n <= 0 */
size_t pcgrl_smb_diversity_scratch_bytes(int32_t h, int32_t w, int32_t n);

/* Pairwise Hamming distances among n caller maps in consecutive groups of `group` maps.  d_scratch (8-byte aligned) and d_sum
 * int64 [n / group] are required; d_scores double [n / group][2], d_nearest, d_nearest_idx int32 [n] and d_pairwise int32
 * [n / group][group][group] may each be NULL. */
int pcgrl_smb_diversity_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t group, void *d_scratch,
                                  int64_t *d_sum, double *d_scores, int32_t *d_nearest, int32_t *d_nearest_idx,
                                  int32_t *d_pairwise, void *stream);

/* The same of the committed maps of every env of h. */
int pcgrl_smb_env_measures(pcgrl_smb_env_handle h, int32_t *d_counts, int32_t *d_match, double *d_forms, double *d_entropy,
                           const double *d_entropy_tab, void *stream);
int pcgrl_smb_env_diversity(pcgrl_smb_env_handle h, int32_t group, void *d_scratch, int64_t *d_sum, double *d_scores,
                            int32_t *d_nearest, int32_t *d_nearest_idx, int32_t *d_pairwise, void *stream);

#ifdef __cplusplus
}
#endif
#endif
