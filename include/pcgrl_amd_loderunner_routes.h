/*
 * pcgrl_amd_loderunner_routes.h -- the routes behind a Lode Runner level's path-length (companion of
 * pcgrl_amd_loderunner.h).
 *
 * A gold whose state is 1 was collected by its own pair of A* searches (envs/probs/loderunner/engine.py:281-308,
 * find_all_golds): to_goal from the landing cell to the gold, to_start from the gold back to the landing cell.  The reference
 * reads both with Node.get_path, which lists the cells from the goal back to the source.  Here
 *
 *   the outward route of such a gold is reversed(to_goal.get_path()[0]):   landing cell ... gold,  gold_dist cells
 *   the return route                is reversed(to_start.get_path()[0]):   gold ... landing cell,  gold_back cells
 *   the tour of a level             is, for each such gold in row-major gold order, its outward then its return route.
 *
 * A gold in state 0, 2 or 3 has no route: one that was never searched, one whose return search failed, and one that an
 * earlier gold's path collected.  The searches' heuristic is not admissible, so a route may be longer than the shortest one.
 *
 * One launch computes everything pcgrl_loderunner_evaluate computes -- the same arguments with the same meaning, the same
 * workspace of pcgrl_loderunner_workspace_bytes -- and the routes:
 *   d_gold_off   int32 [n][gold_cap]: where the gold's outward route starts in the tour; its return route starts at
 *                off + gold_dist.  -1 unless the state is 1
 *   d_gold_back  int16 [n][gold_cap]: the cells of the return route; 0 unless the state is 1
 *   d_coords     int16 [n][route_cap][2]: the tour as (row, column); (-1, -1) past the tour
 *   d_moves      int8 [n][route_cap]: entry k is the move from coords[k] to coords[k + 1] where both lie in the same route:
 *                0 left, 1 right, 2 up, 3 down, 4 down-left, 5 down-right (the reference's Node.action in that order);
 *                -1 at the last cell of each route and past the tour
 *   d_tour_len   int32 [n]: the cells of the whole tour, the sum of gold_dist + gold_back over the golds in state 1
 * d_tour_len, the offsets below gold_cap and the statistics stay complete when route_cap or gold_cap cut what is stored; with
 * route_cap == 0 only the lengths are computed, which is how a caller sizes a second call.
 *
 * Arguments are checked before any HIP call -- PCGRL_EINVAL: what pcgrl_loderunner_evaluate refuses, route_cap < 0,
 * route_cap > 0 with a null d_coords; PCGRL_EUNSUPPORTED: a shape outside 1..16 x 1..32 -- and then one kernel is enqueued on
 * `stream` of the current device: no allocation, no synchronisation, HIP-graph capturable.  Every output but d_stats may be
 * NULL.
 */
#ifndef PCGRL_AMD_LODERUNNER_ROUTES_H
#define PCGRL_AMD_LODERUNNER_ROUTES_H
#include "pcgrl_amd_loderunner.h"

#ifdef __cplusplus
extern "C" {
#endif

int pcgrl_loderunner_routes(const pcgrl_loderunner_config *cfg, int32_t n, const uint8_t *d_grids, void *d_workspace,
                            int64_t workspace_bytes, int32_t gold_cap, int32_t route_cap, double *d_stats, double *d_loss,
                            int32_t *d_play, int8_t *d_gold_state, int16_t *d_gold_dist, int32_t *d_gold_off,
                            int16_t *d_gold_back, int16_t *d_coords, int8_t *d_moves, int32_t *d_tour_len, uint32_t *d_error,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif
