/*
 * pcgrl_amd_archive.h -- the quality-diversity grid archive of libpcgrl_amd.so (companion of pcgrl_amd.h).
 *
 * A MAP-Elites grid on the device: one elite per cell, placed by a behaviour vector, kept when its objective is the best the
 * cell has seen; parents drawn from the occupied cells and mutated, all without a host copy.  It is what the reference's
 * evolution loop does on the host with a [100, ...] grid (evo/evolve.py:1341-1355, :1426-1434; evo/optimizer.py:70-90
 * MEOptimizer.ask; evo/models.py:582-587 DirectEncoding.mutate).  The reference's archive classes come from pyribs and qdpy,
 * which are not part of it: the rules below are this project's own statement, restated in numpy in tests/archive_rules.py, and
 * the kernels are pinned to that bit for bit.  No parity with pyribs' placement at the last bin edge is claimed; a caller who
 * needs a placement of their own passes cell indices.  DESIGN.md section 35 has everything.
 *
 * An archive has a handle of its own and needs no pcgrl_handle.  It has D in 1..4 behaviour axes of dims[j] >= 1 cells each
 * (their product, `cells`, at most 2^20), finite bounds lo[j] < hi[j], maps of L in 1..4096 bytes and T in 1..256 tile types.
 * Per cell it owns in HBM the objective (double), the behaviours (double [D]), an occupied flag (uint8) and the map (L bytes,
 * in a row of L rounded up to 16).
 *
 * Placement of a behaviour x on axis j, in double, in this order, with no fused multiply-add and no reciprocal:
 *
 *   b = min(max(x, lo), hi);   i = (int)(((b - lo) / (hi - lo)) * dims);   i = min(i, dims - 1)
 *
 * and the cell is the C-order flat index over dims.  +-inf clip to the edge cells.  A NaN behaviour or a NaN objective refuses
 * the candidate: status 3, error bit 0, the archive untouched by it.  With d_cells the placement is skipped and an index
 * outside [0, cells) is refused the same way.
 *
 * Insertion: the archive after pcgrl_archive_add equals inserting the n candidates one at a time in batch order under "take
 * the cell if it is empty or the candidate's objective is strictly greater than the occupant's".  Per cell the maximum
 * objective wins, among equal maxima the lowest batch index, and an occupant with an equal objective stays.  Objectives are
 * compared as doubles: -0.0 equals 0.0; -inf takes an empty cell and replaces nothing; +inf is legal.  The stored objective
 * keeps the candidate's bits.
 *
 * Selection and mutation: child c of pcgrl_archive_ask draws its parent uniformly, with replacement, from the occupied cells
 * in ascending cell order; every byte of its copy of the parent's map mutates with probability `rate`, to
 * (t + 1 + r) % T with r uniform in [0, T - 2] (T == 1 mutates nothing).  The draws are a counter-based stream on the
 * splitmix64 finaliser mix():
 *
 *   base   = mix(seed + draw * 0x9e3779b97f4a7c15)
 *   parent = (int)(u(mix(base ^ (c * 0xd1b54a32d192ed03 + 0x8cb92ba72f3d8dd7))) * occupied)
 *   cb     = mix(base ^ (c * 0xd1b54a32d192ed03 + 2 * 0x8cb92ba72f3d8dd7))
 *   q      = mix(cb + (k + 1) * 0x9e3779b97f4a7c15)            for byte k of the map
 *   mutate = u(q) < rate;   r = (int)(u(mix(q ^ 0x8cb92ba72f3d8dd7)) * (T - 1));   u(z) = (z >> 11) * 2^-53
 *
 * in 64-bit wrapping arithmetic.  `draw` lives on the device and advances by one per call that drew, so a captured ask draws
 * fresh children at every replay.  torch's rand / randint streams are not reproduced.  An ask on an empty archive writes
 * nothing and sets error bit 1.
 *
 * pcgrl_archive_create checks its arguments before any HIP call (PCGRL_EINVAL: a null pointer, D outside 1..4, a dim below 1,
 * more than 2^20 cells, a bound that is not finite or lo >= hi, L outside 1..4096, T outside 1..256) and allocates everything
 * the archive will ever need on `device`.  Every other call checks its arguments (a null handle or pointer, n < 1:
 * PCGRL_EINVAL) and then only enqueues kernels and device-to-device copies on `stream`: no allocation, no host
 * synchronisation, HIP-graph capturable.  pcgrl_archive_poll_error alone synchronises.  All data pointers are device
 * pointers; d_maps may have any alignment.  pcgrl_archive_last_error returns this thread's last message of these calls.
 *
 * pcgrl_amd_evo.h makes archives of the same handle type whose payload row is an NCA genome (float32 [P]) instead of a map;
 * every call here but pcgrl_archive_ask serves them with that row where it says d_maps.  Nothing a map archive returns, its
 * image included, differs for it.
 */
#ifndef PCGRL_AMD_ARCHIVE_H
#define PCGRL_AMD_ARCHIVE_H
#include <stddef.h>

#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCGRL_ARCHIVE_MAX_AXES 4
#define PCGRL_ARCHIVE_MAX_CELLS (1 << 20)
#define PCGRL_ARCHIVE_MAX_MAP_BYTES 4096
#define PCGRL_ARCHIVE_MAX_TILES 256
#define PCGRL_ARCHIVE_HEADER_BYTES 128
#define PCGRL_ARCHIVE_IMAGE_VERSION 1

int pcgrl_archive_create(int32_t n_axes, const int32_t *dims, const double *lo, const double *hi, int32_t map_bytes,
                         int32_t n_tiles, int32_t device, void **out);
void pcgrl_archive_destroy(void *archive);

/* Inserts n candidates: d_maps uint8 [n][L], d_objectives double [n], and d_behaviours double [n][D] or d_cells int32 [n] (with
 * d_cells the placement is skipped; d_behaviours, when also given, are stored with the elite, else zeros are).  Outputs:
 * d_status uint8 [n] (0 not the cell's final winner, 1 replaced an occupant, 2 took an empty cell, 3 refused), d_cell int32 [n]
 * (-1 for a refused candidate), d_counts int32 [4] (new, improved, refused, occupied after).  All three are required.  The
 * occupied list and the statistics are rebuilt.  Five launches. */
int pcgrl_archive_add(void *archive, int32_t n, const uint8_t *d_maps, const double *d_objectives, const double *d_behaviours,
                      const int32_t *d_cells, uint8_t *d_status, int32_t *d_cell, int32_t *d_counts, void *stream);

/* The placement alone: d_cell int32 [n], -1 for a vector with a NaN.  Sets no error bit. */
int pcgrl_archive_cells(void *archive, int32_t n, const double *d_behaviours, int32_t *d_cell, void *stream);

/* d_stats double [4]: the occupied count, the maximum and the minimum objective (exact; -inf and +inf when empty) and the sum
 * of the objectives over the occupied cells, in the scan kernel's own fixed order. */
int pcgrl_archive_stats(void *archive, double *d_stats, void *stream);

/* The elites in ascending cell order, the first min(occupied, cap) of them: d_cells int32 [cap], d_objectives double [cap],
 * d_behaviours double [cap][D], d_maps uint8 [cap][L]; each may be NULL.  Rows past the occupied count are not written. */
int pcgrl_archive_elites(void *archive, int32_t cap, int32_t *d_cells, double *d_objectives, double *d_behaviours,
                         uint8_t *d_maps, void *stream);

/* n children: d_out_maps uint8 [n][L] (any alignment), d_out_parent_cell int32 [n] (may be NULL).  rate must be in [0, 1]. */
int pcgrl_archive_ask(void *archive, int32_t n, uint64_t seed, double rate, uint8_t *d_out_maps, int32_t *d_out_parent_cell,
                      void *stream);

/* The image: a header of PCGRL_ARCHIVE_HEADER_BYTES (int32: magic, version, D, dims[4], L, T, 0; double lo[4], hi[4]; uint64
 * draw counter; zeros) then objectives, behaviours, map rows and flags, each section a multiple of 16 bytes.  d_image is
 * 16-byte aligned.  import takes the header's host copy, compares it with the archive before anything is enqueued
 * (PCGRL_EINVAL with the reason: another D, dims, bounds, L, T or version, or image_bytes other than
 * pcgrl_archive_state_bytes), and then overwrites the whole archive. */
int64_t pcgrl_archive_state_bytes(void *archive);
int pcgrl_archive_export(void *archive, void *d_image, void *stream);
int pcgrl_archive_import(void *archive, const void *d_image, int64_t image_bytes, const void *h_header, void *stream);

/* Reads and clears the error word (bit 0 a refused candidate, bit 1 an ask on an empty archive); synchronises `stream`.
 * Negative on a HIP failure. */
int pcgrl_archive_poll_error(void *archive, void *stream);
const char *pcgrl_archive_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
