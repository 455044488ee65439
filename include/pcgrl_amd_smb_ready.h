/*
 * pcgrl_amd_smb_ready.h -- asynchronous stepping of the Super Mario Bros environments of pcgrl_amd_smb_env.h: a budgeted,
 * resumable A* play-through, with the contract pcgrl_step_ready of pcgrl_amd.h has for Sokoban and the 3-D maze.
 *
 * pcgrl_smb_env_step lasts as long as the longest play-through of its launch.  With a budget every launch gives each env at most
 * `budget` search iterations; a search that does not finish is parked in device memory and continues in the next launch, and a
 * status byte per env -- PCGRL_ENV_EMITTED | PCGRL_ENV_BUSY of pcgrl_amd.h -- tells what happened.  Per-env trajectories (maps,
 * positions, statistics, float64 rewards, dones, observations) stay exactly those of pcgrl_smb_env_step, only later; nothing of
 * an unfinished step is ever committed.
 *
 * Contract.  Env i consumes the action of launch t iff it was not busy after launch t - 1 (after a reset: pcgrl_smb_ready_busy);
 * an emitted transition belongs to the last action the env consumed; which launch an env advances in depends on the maps and
 * the budget alone.
 *
 * The launch rules.  A search of a level takes T = it1 + it2 iterations (it2 = 0 when pass 1 wins).  Every launch gives each env B
 * iterations, spent in order on whatever the env searches in that launch.  A search is over when it won, when it == solver_power
 * or when the open list is empty, and it ends in the launch in which its T-th iteration runs: a search whose last iteration uses
 * up the budget is finished, not parked, and pass 2 starts in the same launch with what is left of B.  Per env and launch:
 *   idle                the env consumes its action.  No change, or a change that keeps the cell's solidity: the step completes
 *                       without a search.  Otherwise the search starts; finished -> the step completes, else the env parks a
 *                       PENDING STEP and reports BUSY: its reward / done / stats rows are not written, and the committed state
 *                       is still the one before the step.
 *   pending step        the search resumes; finished -> the step completes, else BUSY.
 *   a completed step    reports EMITTED.  If it ended the episode and auto_reset is set, the next episode is drawn in the same
 *                       launch: the observation is that episode's first, stats the finished episode's, and the new level's
 *                       search starts with the rest of B; unfinished -> PENDING STATISTICS, EMITTED | BUSY.
 *   pending statistics  the search resumes and no action is taken; finished -> statistics and last_loss are set, the env reports
 *                       0 once and takes the next launch's action; else BUSY.
 *   reset               pcgrl_smb_env_reset honours the budget: it abandons whatever the selected envs had in flight (a pending
 *                       step is dropped; nothing of it was committed), and starts the new level's search within the reset
 *                       launch; unfinished -> pending statistics.  The envs outside the mask get no iterations from a reset
 *                       launch and keep what they had parked; their observation rows hold the committed state's.
 *   bad action          an action outside the space taken by an idle env follows pcgrl_smb_env_step's rule (error bit, reward 0,
 *                       the same observation, EMITTED).  The action row of a busy env is not looked at.
 * d_obs rows are written for every env in every launch; a busy env's row holds the observation of the step in flight (of the
 * new episode for pending statistics).  pcgrl_smb_env_get_state returns the committed state: `searches` counts the searches
 * whose result was committed, the iteration counters count every iteration run, and the most one launch spent on an env never
 * exceeds the largest budget used.
 *
 * The park record carries the search loop's words, the env's mode and pending action and the visited set -- not the map: a busy
 * env takes no action, so only a reset or the set and import calls of pcgrl_amd_smb_state.h can change a map under a parked
 * search, and each of them puts the selected envs' park records right in the same launch (a reset and the set call start the
 * new map's search, an import writes idle or a search that starts over).  Results never depend on stale parked state.
 *
 * Every entry point checks its arguments before any HIP call (PCGRL_EINVAL: a null handle or argument, a misaligned observation, a
 * negative budget), enqueues on `stream` only, allocates nothing after the first pcgrl_smb_ready_set_budget and is HIP-graph
 * capturable: a launch is one kernel.
 */
#ifndef PCGRL_AMD_SMB_READY_H
#define PCGRL_AMD_SMB_READY_H
#include "pcgrl_amd.h"
#include "pcgrl_amd_smb_env.h"

#ifdef __cplusplus
extern "C" {
#endif

/* budget >= 1: the first call allocates one park record per env (synchronously); later calls change the budget from the next
 * launch on, and parked searches continue under it.  With a budget set pcgrl_smb_env_step returns PCGRL_EINVAL (it cannot say
 * "busy") and pcgrl_smb_env_reset may leave envs busy.  budget = 0: back to synchronous stepping -- allowed only when no env is
 * busy; it synchronises the device to find out and returns PCGRL_EINVAL otherwise. */
int pcgrl_smb_ready_set_budget(pcgrl_smb_env_handle h, int32_t budget);
/* the budget, 0 without one, -1 for a null handle */
int32_t pcgrl_smb_ready_get_budget(pcgrl_smb_env_handle h);
/* d_status uint8 [n_envs]; d_reward, d_reward64, d_obs, d_done and d_stats may each be NULL as for pcgrl_smb_env_step */
int pcgrl_smb_ready_step(pcgrl_smb_env_handle h, const int32_t *d_actions, int32_t auto_reset, uint8_t *d_obs, float *d_reward,
                         double *d_reward64, uint8_t *d_done, int32_t *d_stats, uint8_t *d_status, void *stream);
/* d_busy uint8 [n_envs]: 1 = the env is busy now (all 0 without a budget) */
int pcgrl_smb_ready_busy(pcgrl_smb_env_handle h, uint8_t *d_busy, void *stream);
/* bytes of one env's park record; -1 for a config that pcgrl_smb_env_create would refuse */
int64_t pcgrl_smb_ready_park_bytes(const pcgrl_smb_env_config *cfg);

#ifdef __cplusplus
}
#endif
#endif
