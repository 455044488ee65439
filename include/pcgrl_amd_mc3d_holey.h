/*
 * pcgrl_amd_mc3d_holey.h -- the 3-D holey dungeon and maze levels of libpcgrl_amd.so (companion of pcgrl_amd.h).
 *
 * One launch evaluates n levels of minecraft_3D_dungeon_holey (problem 0) or minecraft_3D_holey_maze (problem 1): what
 * get_stats of envs/probs/minecraft/minecraft_3D_holey_dungeon_prob.py:87-147 / minecraft_3D_holey_maze_prob.py:71-129 returns
 * for each, the loss ControlWrapper.get_loss would derive from it, and the routes behind the numbers.  A map is the interior,
 * uint8 [Z][Y][X] (the reference's map[z][y][x]), each axis 3..16, of tile ids
 *
 *   0 AIR   1 DIRT   2 CHEST   3 SKULL   4 PUMPKIN          (the maze knows 0 and 1 only)
 *
 * and comes with its two holes, int32 [2][3]: the foot cells of entrance and exit as (z, y, x) in BORDERED coordinates
 * (entrance_coords[0], exit_coords[0]); the head cell is z + 1.  The kernel builds the map HoleyRepresentation3D hands to
 * get_stats (envs/reps/wrappers.py:182-185): a DIRT border of one cell all round, (Z + 2)(Y + 2)(X + 2), the four hole cells
 * AIR.  Every coordinate below is a bordered one.
 *
 * A foot cell is refused unless it lies on one of the four side faces (x = 0 or X + 1 with 1 <= y <= Y, or y = 0 or Y + 1 with
 * 1 <= x <= X) with 1 <= z <= Z - 1 (holey_prob_3D.py:28-31).  A level with a refused hole sets error bit 1, its statistics are
 * -1, its loss is -inf, its routes are empty and no search runs; its neighbours in the batch are not disturbed.
 *
 * The search is helper_3D.run_dijkstra (:422-490) with the passable set {AIR} (maze) or every tile but DIRT (dungeon): a FIFO
 * label-correcting search.  A popped entry is dropped when its cell already has a path no longer than it; a cell without
 * head-room (z + 1 outside the map or not passable) is marked and never becomes a key of `paths`; else the entry is accepted:
 * the cell's path, length and jump count are replaced.  The successors come from helper_3D._passable (:214-319), directions in
 * the order +x, +y, -x, -y, the first matching rule of: walk (foot and head free, floor below); step down (one lower, floor
 * below that, three cells free); step up (a block ahead, two cells free on it and one more above the player); jump over a gap
 * (five cells free ahead, one more above the player, the landing two cells away in the map) onto a landing at the same level,
 * one up (if z + 3 is inside the map) or one down, tried in that order -- a gap with no landing gives nothing.  A path's length
 * is its number of tiles, the traversed tiles of a step or jump included (a move adds 1, 2 or 3); `jumps` is the jump count of
 * the accepted path.  The keys of `paths` keep the order of their FIRST acceptance.
 *
 * Dungeon statistics (int32 [6]): 0 regions (6-neighbour regions of AIR ONLY, on the bordered map with its holes),
 * 1 path-length, 2 chests, 3 enemies (SKULL + PUMPKIN), 4 nearest-enemy, 5 n_jump.  nearest-enemy is the smallest length of a
 * path from the entrance foot to an enemy that is a key of `paths`, 0 without one; the enemies are tried SKULLs first, then
 * PUMPKINs, each in z-major, y, x order, with a strict `<`, so the first of equals gives the route.  With a chest, the FIRST
 * chest in that order counts: path-length = len(entrance -> chest) + len(chest -> exit foot), a leg that is not reached
 * counting 0, and n_jump the sum of the two legs' jump counts.  The second search starts on the chest cell whether or not
 * anything can stand there (only head-room is asked of it, as of any cell).  The entrance search runs if the level has an
 * enemy or a chest, the chest search if it has a chest.
 *
 * Maze statistics (int32 [4]): 0 regions, 1 path-length, 2 connected-path-length, 3 n_jump, from one search from the entrance.
 * connected-path-length is the length of the exit foot's path, -1 if it has none; n_jump its jump count, else 0.  path-length
 * is that of the CURRENT map: the number of tiles remove_stacked_path_tiles leaves (helper_3D.py:657-675: a tile goes when the
 * tile below it is in the path) of the first longest path in the order of first acceptance.  The reference returns there the
 * value of its previous call (line 92 reads path_coords before line 93 sets it); a second call on the same map returns this
 * one.
 *
 * The loss: for each statistic in the order above, -(distance to its target) * weight, each term rounded to double and then
 * added, no fused multiply-add.  A target is the zero-loss interval [trg_lo, trg_hi] (a tuple target (lo, hi) of the reference
 * means the integers of arange(lo, hi)).
 *
 * The queue is a ring of Q entries per search, Q the power of two >= 8 * (Z + 2)(Y + 2)(X + 2).  The live entries belong to two
 * consecutive depths (numbers of moves from the start), each at most four per accepted pop of the depth before; were no cell
 * accepted twice within one depth that is 4 * cells + 4 * cells.  A cell can be accepted again within a depth, so Q is a
 * capacity: a level whose push finds the ring full sets error bit 2 and answers as a refused level does.  An entry that the
 * cell's accepted length already beats is dropped when it would be pushed; that is exact because that length only shrinks.
 *
 * pcgrl_mc3d_holey_evaluate checks its arguments before any HIP call -- PCGRL_EINVAL: null cfg, grids, holes or stats, n < 1,
 * route_cap < 0, a problem other than 0 or 1, a workspace that is null, not 16-byte aligned or smaller than one block's slot
 * (pcgrl_mc3d_holey_workspace_bytes(1, ...)); PCGRL_EUNSUPPORTED: an axis outside 3..16 -- and then only enqueues one kernel
 * on `stream` of the current device: no allocation, no synchronisation, HIP-graph capturable.  It launches
 * min(n, workspace_bytes / slot) workgroups, which stride over the levels.  d_grids may have any alignment.  The workspace need
 * not be cleared.
 *
 * Outputs (device pointers; every one but d_stats may be NULL, and a NULL output is not written):
 *   d_stats      int32 [n][6] (dungeon) or [n][4] (maze)
 *   d_loss       double [n]
 *   d_play       int32 [n][12]: 0 the searches that ran (bit 0 from the entrance, bit 1 from the chest); 1, 2 the accepted
 *                pops and the queue entries the reference makes (the start included) of the first; 3, 4 of the second;
 *                5..7 (x, y, z) of the dungeon's first chest or of the maze's farthest cell; 8..10 of the dungeon's nearest
 *                enemy; -1 where there is none; 11 is 0.
 *   d_error      uint32 [n]: bit 0 a tile id the problem does not know was read as DIRT, bit 1 a refused hole, bit 2 the ring
 *   d_coords     int16 [n][route_cap][3], (x, y, z) as the reference's path tuples, (-1, -1, -1) past the end: the dungeon's
 *                ordered main route path_c + path_d, the maze's ordered connected path.  Ignored when route_cap is 0.
 *   d_route_len  int32 [n]: that route's number of tiles, whatever route_cap cuts
 *   d_leg_len    int32 [n][2]: the dungeon's two legs (0, 0 for the maze)
 *   d_coords2, d_route2_len   the same for the dungeon's ordered_e_path (the nearest enemy's route) and the maze's ordered_path
 *                (the first longest path)
 *   d_overlay, d_overlay2   uint8 [n][Z+2][Y+2][X+2], 1 on the tiles remove_stacked_path_tiles leaves of the first and of
 *                the second route (the reference's lists are unordered: compare as sets)
 */
#ifndef PCGRL_AMD_MC3D_HOLEY_H
#define PCGRL_AMD_MC3D_HOLEY_H
#include <stddef.h>

#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCGRL_MC3D_HOLEY_MAX_STATS 6
#define PCGRL_MC3D_HOLEY_PLAY 12
#define PCGRL_MC3D_HOLEY_DUNGEON 0
#define PCGRL_MC3D_HOLEY_MAZE 1

typedef struct pcgrl_mc3d_holey_config {
  int32_t problem; /* 0 dungeon, 1 maze */
  int32_t z, y, x; /* the interior, 3..16 each */
  /* per statistic, in the problem's order: the weight and the zero-loss interval of the loss */
  double weight[PCGRL_MC3D_HOLEY_MAX_STATS], trg_lo[PCGRL_MC3D_HOLEY_MAX_STATS], trg_hi[PCGRL_MC3D_HOLEY_MAX_STATS];
} pcgrl_mc3d_holey_config;

/* bytes of the workspace for `blocks` workgroups: per workgroup two rings of Q * 8 bytes and, above 1024 bordered cells, two
 * copies of the per-cell search state (9 bytes a cell, each array rounded up to 16); negative outside the limits or blocks < 1 */
int64_t pcgrl_mc3d_holey_workspace_bytes(int32_t blocks, int32_t z, int32_t y, int32_t x);

int pcgrl_mc3d_holey_evaluate(const pcgrl_mc3d_holey_config *cfg, int32_t n, const uint8_t *d_grids, const int32_t *d_holes,
                              void *d_workspace, int64_t workspace_bytes, int32_t route_cap, int32_t *d_stats, double *d_loss,
                              int32_t *d_play, uint32_t *d_error, int16_t *d_coords, int32_t *d_route_len, int32_t *d_leg_len,
                              int16_t *d_coords2, int32_t *d_route2_len, uint8_t *d_overlay, uint8_t *d_overlay2, void *stream);

#ifdef __cplusplus
}
#endif
#endif
