/*
 * pcgrl_amd_microstructure.h -- microstructure levels of libpcgrl_amd.so (companion of pcgrl_amd.h).
 *
 * One launch evaluates n microstructure levels: what MicroStructureProblem.get_stats returns for each
 * (envs/probs/microstructure/microstructure_prob.py:107-119 -> envs/helper.py:278-318 calc_tortuosity), the loss
 * ControlWrapper.get_loss would derive from it, and the per-region record behind both statistics.  A map is uint8 [H][W] of
 * tile ids
 *
 *   0 empty   1 solid                                            (microstructure_prob.py:60-61)
 *
 * and the statistics come in get_stats' order:
 *
 *   0 path-length   1 tortuosity
 *
 * The regions (4-connected sets of empty cells) are visited in the row-major order of their first cell.  Per region: a
 * breadth-first flood from the first cell, the first cell in row-major order at the greatest distance (the far cell; the cell
 * itself for a one-cell region), a second flood from the far cell whose greatest distance is the region's d; l2 is the
 * Euclidean distance from the first cell to the far cell, 0 replaced by 1; tort = d / l2.  path-length is the largest d;
 * tortuosity is np.mean over the regions' tort in visit order -- numpy's pairwise sum, then one division by the count -- and
 * both are 0 for a map without an empty cell.
 *
 * Stepping microstructure environments is not part of the engine: pcgrl_create does not know the problem, and nothing here
 * needs a pcgrl_handle.
 *
 * pcgrl_microstructure_evaluate checks its arguments before any HIP call -- PCGRL_EINVAL: null cfg, grids or stats, n < 1,
 * region_cap < 0; PCGRL_EUNSUPPORTED: a shape outside 1..64 x 1..64 -- and then only enqueues one kernel on `stream` of the
 * current device: no allocation, no workspace, no synchronisation, HIP-graph capturable.  d_grids may have any alignment.
 *
 * Outputs (device pointers; every one but d_stats may be NULL):
 *   d_stats        double [n][2]: every value exactly the double of the reference's Python value
 *   d_loss         double [n]: sum over the statistics with has_trg of -(distance of the value to [trg_lo, trg_hi]) * weight,
 *                  in order, each term one multiplication and one addition in double
 *   d_regions      int32 [n]: the number of regions, the mean's divisor
 *   d_region_rec   int16 [n][region_cap][5]: per region in visit order start row, start column, far row, far column, d;
 *                  all five -1 past the last region
 *   d_region_tort  double [n][region_cap]: the region's tort; 0 past the last region
 *   d_error        uint32 [n]: bit 0 = a tile id above 1 was read as solid
 * The statistics and d_regions stay complete when region_cap is smaller than the number of regions.
 *
 * The measures and the pairwise Hamming diversity of such maps: the quantities, the rules and the order of the double
 * operations are those of pcgrl_amd_measures.h -- read that header for d_counts, d_match, d_forms, d_entropy / d_entropy_tab,
 * d_sum, d_scores, d_nearest, d_nearest_idx and d_pairwise -- with T = 2 tile types (d_counts is int32 [n][2], d_forms double
 * [n][7]) and n_cells = h * w; tile ids are masked to 1 bit and set no error.  The argument lists and the checks are those of
 * pcgrl_amd_loderunner_measures.h, with this header's shape range.
 */
#ifndef PCGRL_AMD_MICROSTRUCTURE_H
#define PCGRL_AMD_MICROSTRUCTURE_H
#include <stddef.h>

#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCGRL_MICROSTRUCTURE_STATS 2

typedef struct pcgrl_microstructure_config {
  int32_t h, w; /* 1..64 x 1..64 */
  int32_t has_trg[PCGRL_MICROSTRUCTURE_STATS];
  double weight[PCGRL_MICROSTRUCTURE_STATS];
  double trg_lo[PCGRL_MICROSTRUCTURE_STATS], trg_hi[PCGRL_MICROSTRUCTURE_STATS]; /* the zero-loss interval, both ends included */
} pcgrl_microstructure_config;

int pcgrl_microstructure_evaluate(const pcgrl_microstructure_config *cfg, int32_t n, const uint8_t *d_grids, int32_t region_cap,
                                  double *d_stats, double *d_loss, int32_t *d_regions, int16_t *d_region_rec,
                                  double *d_region_tort, uint32_t *d_error, void *stream);

/* The measures of n caller maps.  d_counts int32 [n][2] and d_match int32 [n][3] are required; d_forms double [n][7] and
 * d_entropy double [n] may each be NULL, and only with d_entropy is d_entropy_tab (h * w + 2 doubles, T = 2) read. */
int pcgrl_microstructure_measures_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t *d_counts,
                                            int32_t *d_match, double *d_forms, double *d_entropy, const double *d_entropy_tab,
                                            void *stream);

/* bytes of the scratch the diversity call needs for n maps of h x w (their bit-plane image and one nearest-map key each:
 * 8 * (ceil(h * w / 64) + 1) per map); 0 for an unsupported shape or n <= 0 */
size_t pcgrl_microstructure_diversity_scratch_bytes(int32_t h, int32_t w, int32_t n);

/* Pairwise Hamming distances among n caller maps in consecutive groups of `group` maps.  d_scratch (8-byte aligned) and d_sum
 * int64 [n / group] are required; d_scores double [n / group][2], d_nearest, d_nearest_idx int32 [n] and d_pairwise int32
 * [n / group][group][group] may each be NULL. */
int pcgrl_microstructure_diversity_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t group,
                                             void *d_scratch, int64_t *d_sum, double *d_scores, int32_t *d_nearest,
                                             int32_t *d_nearest_idx, int32_t *d_pairwise, void *stream);

#ifdef __cplusplus
}
#endif
#endif
