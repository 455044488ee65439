/*
 * pcgrl_amd_solutions.h -- Sokoban solutions of libpcgrl_amd.so (companion of pcgrl_amd.h).
 *
 * The engine reports `sol-length` for every sokoban map it steps or scores; these entry points hand out the solution that
 * number is the length of: the move list SokobanProblem.get_stats leaves in stats["solution"] (sokoban_prob.py:178, found by
 * _run_game :99-148: BFSAgent, then AStarAgent with balance 1, 0.5, 0, each to solver_power iterations, the first win ends
 * it), move for move.  A move is coded as its index in the reference's `directions` (engine.py:3):
 *
 *   0 = {"x": -1, "y": 0}   1 = {"x": 1, "y": 0}   2 = {"x": 0, "y": -1}   3 = {"x": 0, "y": 1}
 *
 *   problem   the solution
 *   sokoban   the winning node's Node.getActions (engine.py:27-35), root first; `sol-length` moves.
 *   binary, zelda, 3-D maze   PCGRL_EUNSUPPORTED: no solver, no action list (their paths: pcgrl_amd_paths.h, the overlay).
 *
 * The solution is a function of the map and cfg.solver_power alone: the state of the statistics (stale after pcgrl_update),
 * the representation wrappers and a solver budget (pcgrl_set_solver_budget) do not matter -- with a budget set the call still
 * runs its searches to the end, on the synchronous workspace pool, and no env's busy state changes.  Every entry point below
 * only enqueues a kernel on `stream` (HIP-graph capturable; the one exception is the growth of the workspace pool, as in
 * pcgrl_stats_for_grids_h: synchronous, once, never while `stream` is being captured -- pcgrl_reserve_solver_pool beforehand
 * avoids it), checks its handle, its pointers, cap >= 1 and n >= 0 (PCGRL_EINVAL) and the problem (PCGRL_EUNSUPPORTED) before
 * any HIP call, runs on the engine's device and restores the caller's.  A level beyond the device solver's limits raises
 * error bit 2 (pcgrl_poll_error), as in the step kernels.
 *
 * Outputs (device pointers):
 *   d_moves     int8 [n][cap]: the first min(len, cap) moves in playing order; every later byte is -1
 *   d_len       int32 [n]: the full length, also where it exceeds cap; 0 when the solver ran and no stage won (the reference
 *               returns []); -1 when the solver's precondition does not hold -- exactly one player, crates == targets > 0, one
 *               region (sokoban_prob.py:172-177) -- and the reference's statistics have no "solution" key
 *   d_dist_win  int32 [n], or NULL: `dist-win` as the statistics define it (0 on a win, else the heuristic of the last stage's
 *               best node; H * W * (H + W) without the precondition)
 */
#ifndef PCGRL_AMD_SOLUTIONS_H
#define PCGRL_AMD_SOLUTIONS_H
#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* an upper bound on len: cfg.solver_power (a popped node's depth cannot exceed the iterations run); 0 for the problems
 * without a solver; -1 on a null handle */
int32_t pcgrl_solution_capacity(pcgrl_handle h);

/* The solution of the CURRENT map of every env of h (n = the engine's batch): what env.unwrapped._prob.get_stats(map)
 * ["solution"] holds (sokoban_prob.py:160-180). */
int pcgrl_solutions(pcgrl_handle h, int32_t cap, int8_t *d_moves, int32_t *d_len, int32_t *d_dist_win, void *stream);

/* The same for n caller maps, uint8 [n][H][W] tile ids of the map shape of h (SokobanProblem._run_game on any map).  n is
 * independent of the engine's batch, as with pcgrl_stats_for_grids_h; n == 0 is a no-op. */
int pcgrl_solutions_for_grids(pcgrl_handle h, int32_t n, const uint8_t *d_grids, int32_t cap, int8_t *d_moves, int32_t *d_len,
                              int32_t *d_dist_win, void *stream);

#ifdef __cplusplus
}
#endif
#endif
