/*
 * pcgrl_amd_smb_rollout.h -- open-loop rollouts of the Super Mario Bros environments of pcgrl_amd_smb_env.h: K steps of every
 * env in one launch, and action_space.sample() drawn on the device.
 *
 * pcgrl_smb_env_step lasts as long as the longest play-through of its launch, so K launches cost the sum over steps of the
 * batch's longest search.  A rollout steps each env K times inside one kernel with no boundary in between, so the launch costs
 * the largest, over envs, of the env's own K steps.  It is for actions that do not depend on the observations: replaying
 * recorded episodes, random-action loops, repair trajectories.  Per env the K transitions -- maps, positions, statistics,
 * float64 rewards, dones, observations, the finished episodes, the RNG streams and every counter of pcgrl_smb_env_get_state --
 * are bit for bit those of K calls of pcgrl_smb_env_step.
 *
 *   actions   d_actions int32 [n_steps][n_envs], or NULL: drawn on the device.  The action of env i at step k of a call is
 *               floor(r * n_actions / 2^64),  r = mix64(mix64(seed + (c + k) * 0x9e3779b97f4a7c15)
 *                                                         ^ (i * 0xd1b54a32d192ed03 + 0x8cb92ba72f3d8dd7))
 *             with mix64 the splitmix64 finaliser -- the function pcgrl_sample_actions of pcgrl_amd.h uses -- and c the handle's
 *             draw counter: 0 after pcgrl_smb_env_create, kept in device memory, read by every env of a launch and then advanced
 *             by n_steps (by 1 by pcgrl_smb_env_sample_actions), on the device and in stream order.  A captured call therefore
 *             draws fresh actions at every replay, and a rollout of K drawn steps takes the actions of K times
 *             [pcgrl_smb_env_sample_actions, pcgrl_smb_env_step].  A call with d_actions given leaves the counter alone.  The
 *             counter is synthetic input: it is not part of the image of pcgrl_amd_smb_state.h, as pcgrl_amd.h says of the
 *             engine's.  d_actions_out int32 [n_steps][n_envs] receives the actions taken.
 *   bad action  an action outside the space follows pcgrl_smb_env_step's rule for that step -- the error bit, reward 0, not done,
 *             the same statistics, the env as it was -- and the env goes on with step k + 1.
 *   rows      d_reward (float), d_reward64 (double), d_done uint8 [n_steps][n_envs], d_stats int32 [n_steps][n_envs][9]: row k is
 *             what step k's call would have written.
 *   obs       obs_mode 0: none (d_obs is not looked at).  1: d_obs [n_envs][obs_bytes], the observation after the last step.
 *             2: d_obs [n_steps][n_envs][obs_bytes], row k what step k would have returned; at an episode end with auto_reset
 *             that is the new episode's first observation.  d_obs must be 16-byte aligned.
 *   episodes  the episodes finished inside this launch, per env: d_ep_count int32 [n_envs], d_ep_return_sum double [n_envs] (the
 *             returns added in the order the episodes finished, starting from 0.0), d_ep_length_sum int64 [n_envs],
 *             d_ep_stats_sum int64 [n_envs][9].  An episode counts wherever pcgrl_smb_env_step would latch it: without
 *             auto_reset that is every step past the end, as pcgrl_smb_env_get_last_episode's count does.
 *
 * Every output pointer may be NULL.  PCGRL_EINVAL, before any HIP call: a null handle, n_steps < 1, n_steps * n_envs above
 * 2^31 - 1, obs_mode outside 0..2, obs_mode != 0 with a null or misaligned d_obs, a null d_actions of
 * pcgrl_smb_env_sample_actions, and for the rollout a solver budget set on the handle (pcgrl_amd_smb_ready.h): like
 * pcgrl_smb_env_step it cannot say "busy".  A call enqueues one kernel on `stream`, allocates nothing (pcgrl_smb_env_create allocates the draw
 * counter) and is HIP-graph capturable.
 */
#ifndef PCGRL_AMD_SMB_ROLLOUT_H
#define PCGRL_AMD_SMB_ROLLOUT_H
#include "pcgrl_amd_smb_env.h"

#ifdef __cplusplus
extern "C" {
#endif

int pcgrl_smb_env_rollout(pcgrl_smb_env_handle h, const int32_t *d_actions /* NULL: drawn */, uint64_t seed,
                          int32_t n_steps, int32_t auto_reset, uint8_t *d_obs, int32_t obs_mode,
                          float *d_reward, double *d_reward64, uint8_t *d_done, int32_t *d_stats,
                          int32_t *d_actions_out, int32_t *d_ep_count, double *d_ep_return_sum,
                          int64_t *d_ep_length_sum, int64_t *d_ep_stats_sum, void *stream);
/* d_actions int32 [n_envs]: one draw for every env; the draw counter advances by 1 */
int pcgrl_smb_env_sample_actions(pcgrl_smb_env_handle h, int32_t *d_actions, uint64_t seed, void *stream);
/* 7 narrow, 11 turtle, -1 on a null handle */
int32_t pcgrl_smb_env_num_actions(pcgrl_smb_env_handle h);

#ifdef __cplusplus
}
#endif
#endif
