/*
 * pcgrl_amd_multiagent.h -- multi-agent turtle stepping of libpcgrl_amd.so (companion of pcgrl_amd.h).
 *
 * The reference's n_agents experiments (configs/experiment/n_agents.yaml: representation turtle, multiagent.n_agents 1..3,
 * show_agents on / off): MultiAgentWrapper over MultiAgentTurtleRepresentation, optionally under ShowAgentRepresentation
 * (wrappers.py:697-736, reps/wrappers.py:189-231, :616-651).  A agents walk and edit ONE map:
 *
 *   reset    the turtle's own reset, then the spawn draw from the representation's generator: A different cells
 *            (Generator.choice(n_cells, A, replace=False)); a map with fewer cells than agents puts everybody on cell 0.
 *   round    the agents take their sub-steps in index order.  A sub-step is a whole PcgrlEnv.step from the agent's own
 *            position on the map the agents before it have edited: iteration + 1, the turtle update, new statistics when the
 *            map changed, reward = the change of the loss (so the rewards of a round telescope), done = iteration >
 *            max_iterations or changes > max_changes, and the agent's observation: the crop around its new position of the
 *            map right after its own sub-step.  An absent agent (action -1) and an agent that has reported done since the
 *            reset take no sub-step.  The round after which every agent has reported done ends the episode.
 *   show_agents  one more channel behind the one-hot ones: 1 on every map cell that holds an agent at that moment, cropped
 *            like the map, 0 outside it.
 *
 * pcgrl_ma_attach turns a 2-D turtle engine of the binary or zelda problem into a multi-agent one.  From then on the
 * single-agent stepping entry points (pcgrl_step*, pcgrl_rollout*, pcgrl_update, pcgrl_reset, pcgrl_observe) answer
 * PCGRL_EINVAL; pcgrl_get_state, pcgrl_get_rng_state, pcgrl_export_state / pcgrl_import_state, the episode queries,
 * pcgrl_paths and pcgrl_poll_error keep working (the position pcgrl_get_state reports is the wrapped turtle's own, which
 * nothing uses).  Every entry point below checks its arguments before any HIP call, only enqueues work on `stream`
 * (HIP-graph capturable), runs on the engine's device and restores the caller's.
 *
 * Per-env side state (what pcgrl_ma_get_state / pcgrl_ma_set_state carry, next to the engine's own state image):
 *   pos         int32  [N][A][2]  (row, col) of every agent
 *   side        uint32 [N][4]     done bits since the reset (bit i = agent i), then the generator's kept 32-bit half: flag, value
 *   last_stats  int32  [N][A][PCGRL_MAX_STATS]  the statistics after the agent's last sub-step (after a reset: the reset's)
 */
#ifndef PCGRL_AMD_MULTIAGENT_H
#define PCGRL_AMD_MULTIAGENT_H
#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCGRL_MA_MAX_AGENTS 8

/* Once per engine, 1 <= n_agents <= 8.  PCGRL_EUNSUPPORTED with a message: another representation than turtle (the reference
 * itself fails on them), sokoban and the 3-D maze, static tiles, action patches, control metrics, a solver budget, and
 * show_agents with one agent (the reference raises).  PCGRL_EINVAL: a second attach, n_agents out of range, statistics left
 * stale by pcgrl_update. */
int pcgrl_ma_attach(pcgrl_handle h, int32_t n_agents, int32_t show_agents);

/* 1 after pcgrl_ma_attach, else 0; -1 on a null handle */
int32_t pcgrl_ma_attached(pcgrl_handle h);

/* the observation of ONE agent: (obs_window rows, obs_window columns, n_tiles + 1 (+ 1 with show_agents)) */
int pcgrl_ma_obs_shape(pcgrl_handle h, int32_t shape_out[4], int32_t *ndim_out);

/* Resets the envs of d_mask (uint8 [N], NULL = all): a new map and the spawn draw from the env's generators, or -- both or
 * neither -- injected maps d_init_grids (uint8 [N][H][W]) with injected positions d_init_pos (int32 [N][A][2]), which draw
 * nothing; a position outside the map is clamped to it and a tile id outside the problem's reads as tile 0, either raises the
 * error bit.  d_obs (or NULL): uint8 [N][A][obs_bytes], the observations of all agents, each cropped at its own cell -- the rows
 * of ALL envs are written, those outside d_mask with their current observations. */
int pcgrl_ma_reset(pcgrl_handle h, const uint8_t *d_mask, const uint8_t *d_init_grids, const int32_t *d_init_pos,
                   uint8_t *d_obs, void *stream);

/* One round of every env in one launch.  Outputs other than d_actions may be NULL.
 *   an agent that is absent (-1) or done takes no sub-step whatever its action: reward 0, done = its done bit, its last
 *   statistics; its observation row is left unwritten.
 *   d_done_all is 1 in the round after which every agent's bit is set.  With auto_reset that round ends with the reset inside
 *   the launch: rewards, dones and statistics are the finished round's, all A observation rows the first of the new episode,
 *   and the episode is latched for pcgrl_get_last_episode / pcgrl_reduce_episodes (return = the sum over the agents, length =
 *   iteration).
 *   an action that is neither -1 nor inside Discrete(4 + n_tiles) edits nothing and raises the error bit (pcgrl_poll_error). */
int pcgrl_ma_step(pcgrl_handle h, const int32_t *d_actions /* int32 [N][A], -1 = the agent is absent this round */,
                  int32_t auto_reset, uint8_t *d_obs /* [N][A][obs_bytes] */, float *d_reward /* float [N][A] */,
                  uint8_t *d_done /* uint8 [N][A] */, int32_t *d_stats /* int32 [N][A][n_stats], after each sub-step */,
                  uint8_t *d_done_all /* uint8 [N] */, void *stream);

/* the A observations of every env's current state, uint8 [N][A][obs_bytes] */
int pcgrl_ma_observe(pcgrl_handle h, uint8_t *d_obs, void *stream);

/* the side state (see the head of this file); any pointer may be NULL.  pcgrl_ma_set_state: the envs of d_mask; positions are
 * clamped to the map (and the error bit raised). */
int pcgrl_ma_get_state(pcgrl_handle h, int32_t *d_pos, uint32_t *d_side, int32_t *d_last_stats, void *stream);
int pcgrl_ma_set_state(pcgrl_handle h, const uint8_t *d_mask, const int32_t *d_pos, const uint32_t *d_side,
                       const int32_t *d_last_stats, void *stream);

#ifdef __cplusplus
}
#endif
#endif
