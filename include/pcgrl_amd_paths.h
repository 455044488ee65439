/*
 * pcgrl_amd_paths.h -- solution paths of libpcgrl_amd.so (companion of pcgrl_amd.h).
 *
 * The engine reports `path-length` for every map it steps or scores; these entry points say WHICH path that number
 * measures: the ordered cell list the reference keeps for rendering (Problem.render draws it over the level), cell for cell,
 * and optionally the path as a mask.  Cells are (row, col), the reference's [y, x].
 *
 *   problem   the path                                                                       longest
 *   binary    BinaryProblem.get_stats' path_coords (binary_prob.py:152-158): helper.py:255-276  n_cells
 *             calc_longest_path(get_path=True) -> :321-426 get_path_coords.  path-length + 1
 *             cells from the far end of the longest shortest path back to its start; empty
 *             when path-length is 0.
 *   zelda     ZeldaCtrlProblem.get_stats' self.path with render_path (zelda_ctrl_prob.py:       2 * n_cells
 *             153-165): key -> player, then door -> key, without the cells of the player, the
 *             key and the door; empty unless there is exactly one of each.  A half whose
 *             target is walled in is empty, the other half stays.
 *   sokoban   PCGRL_EUNSUPPORTED: its "solution" is an action list out of a transient search, not a path
 *             (pcgrl_amd_solutions.h hands that list out).
 *   3-D maze  PCGRL_EUNSUPPORTED: the path is already the overlay channel of the observation (pcgrl_observe).
 *
 * The path is a function of the map alone: the state of the statistics (stale after pcgrl_update) and the representation
 * wrappers do not matter.  Every entry point below only enqueues kernels on `stream` (HIP-graph capturable), checks its
 * handle, its pointers, cap >= 1 and n >= 0 (PCGRL_EINVAL) and the problem (PCGRL_EUNSUPPORTED) before any HIP call, runs on
 * the engine's device and restores the caller's.
 *
 * Outputs (device pointers):
 *   d_path     int16 [n][cap][2]: the first min(len, cap) cells; every later row is (-1, -1)
 *   d_len      int32 [n]: the full length, also where it exceeds cap
 *   d_overlay  uint8 [n][H][W], or NULL: 1 on every path cell (those past cap included), 0 elsewhere
 */
#ifndef PCGRL_AMD_PATHS_H
#define PCGRL_AMD_PATHS_H
#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* an upper bound on len: n_cells (binary), 2 * n_cells (zelda); 0 for the problems without a path; -1 on a null handle */
int32_t pcgrl_path_capacity(pcgrl_handle h);

/* The path of the CURRENT map of every env of h (n = the engine's batch): what env.unwrapped._prob.path_coords (binary_prob.py:
 * 152-158) / .path (zelda_ctrl_prob.py:153-165) hold after get_stats on that map. */
int pcgrl_paths(pcgrl_handle h, int32_t cap, int16_t *d_path, int32_t *d_len, uint8_t *d_overlay, void *stream);

/* The same for n caller maps, uint8 [n][H][W] tile ids of the problem and map shape of h (helper.py:255-276 / :321-426 on any
 * map).  n is independent of the engine's batch, as with pcgrl_stats_for_grids_h; n == 0 is a no-op. */
int pcgrl_paths_for_grids(pcgrl_handle h, int32_t n, const uint8_t *d_grids, int32_t cap, int16_t *d_path, int32_t *d_len,
                          uint8_t *d_overlay, void *stream);

#ifdef __cplusplus
}
#endif
#endif
