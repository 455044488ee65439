/*
 * pcgrl_amd_smb_env.h -- stepping Super Mario Bros environments of libpcgrl_amd.so (companion of pcgrl_amd_smb.h).
 *
 * What make_env(cfg) of the reference does for smb with the narrow or the turtle representation, for n_envs environments on
 * one device: reset (envs/pcgrl_env.py:158-188), the representation's update (reps/narrow_rep.py, reps/turtle_rep.py), the
 * statistics of pcgrl_amd_smb.h, reward = loss - last_loss in double (control_wrappers.py:216-244), done
 * (iteration > max_iterations, or changes > max_changes when max_changes >= 0), the cropped one-hot observation
 * (wrappers.py:407-437) and the automatic reset.  The engine of pcgrl_amd.h is not involved: pcgrl_create still refuses smb.
 *
 *   actions   narrow: 0..6 = the tile written at the scan position (row-major; the first cell is visited twice).
 *             turtle: 0..3 move by (-1,0), (1,0), (0,-1), (0,1) on (row, col), clamped; 4..10 write tile a - 4.
 *             An action outside the space sets an error bit (pcgrl_smb_env_poll_error: PCGRL_EACTION) and leaves the env as it
 *             was for that step: reward 0, not done, the same observation.
 *   obs       uint8 [n_envs][obs_window[0]][obs_window[1]][8]: channel 0 = outside the map, channel 1 + tile inside; the window
 *             is centred on the position (row pos - oh / 2 is the first).
 *   stats     int32 [n_envs][9] in pcgrl_amd_smb.h's order: the statistics after the step -- of the finished episode where the
 *             step ended one.  They are recomputed only when the written tile differs from the old one, and the A* play-through
 *             runs only when the edit changed the cell's solidity (solid, brick, question, tube against empty, enemy, coin):
 *             otherwise the level the play-through sees is the same and its four statistics keep their values -- exactly.
 *   reset     d_mask (uint8 [n_envs], NULL = all) selects the envs; d_init_grids (uint8 [n_envs][h][w]) replaces the drawn map
 *             and draws nothing from the streams, d_init_pos (int32 [n_envs][2], turtle, clamped into the map) its start.  This
 *             is also the way to set a state.  A reset always runs the play-through.
 *
 * Every call checks its arguments before any HIP call -- PCGRL_EINVAL: null or misshaped arguments, an observation pointer
 * that is not 16-byte aligned, a workspace smaller than pcgrl_smb_env_workspace_bytes; PCGRL_EUNSUPPORTED: a shape outside
 * 4..16 x 1..128, solver_power outside 1..16000, the wide representation (the reference's wide fails on a non-square map), an
 * obs_window entry outside 1..255 (the reference keeps the pad as int8 and fails above) -- and then enqueues one kernel on
 * `stream`: no allocation, no synchronisation, HIP-graph capturable.  pcgrl_smb_env_create allocates the per-env state; the
 * search workspace belongs to the caller and must outlive the handle.  pcgrl_smb_env_seed and pcgrl_smb_env_poll_error
 * synchronise the device.
 */
#ifndef PCGRL_AMD_SMB_ENV_H
#define PCGRL_AMD_SMB_ENV_H
#include "pcgrl_amd_smb.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pcgrl_smb_env_config {
  int32_t h, w;           /* 4..16 x 1..128 */
  int32_t representation; /* PCGRL_REP_NARROW or PCGRL_REP_TURTLE */
  int32_t obs_window[2];  /* 1..255 each; the reference's default is (2h, 2w) */
  int32_t max_iterations; /* h * w * max_board_scans + 1 */
  int32_t max_changes;    /* max(int(change_percentage * h * w), 1), or -1 for none */
  int32_t solver_power;   /* 1..PCGRL_SMB_MAX_SOLVER_POWER */
  int32_t n_envs;
  int32_t has_trg[PCGRL_SMB_STATS];
  double weight[PCGRL_SMB_STATS];
  double trg_lo[PCGRL_SMB_STATS], trg_hi[PCGRL_SMB_STATS]; /* the zero-loss interval, both ends included */
} pcgrl_smb_env_config;

typedef struct pcgrl_smb_env *pcgrl_smb_env_handle;

/* bytes of search workspace (pcgrl_smb_workspace_bytes of n_envs levels) and of one env's observation; -1 for a config that
 * pcgrl_smb_env_create would refuse */
int64_t pcgrl_smb_env_workspace_bytes(const pcgrl_smb_env_config *cfg);
int64_t pcgrl_smb_env_obs_bytes(const pcgrl_smb_env_config *cfg);

int pcgrl_smb_env_create(const pcgrl_smb_env_config *cfg, int32_t device, void *d_workspace, int64_t workspace_bytes,
                         pcgrl_smb_env_handle *out);
void pcgrl_smb_env_destroy(pcgrl_smb_env_handle h);
/* env i gets numpy's PCG64(SeedSequence(seeds[i])) for both streams */
int pcgrl_smb_env_seed(pcgrl_smb_env_handle h, const uint64_t *seeds);
int pcgrl_smb_env_reset(pcgrl_smb_env_handle h, const uint8_t *d_mask, const uint8_t *d_init_grids, const int32_t *d_init_pos,
                        uint8_t *d_obs, void *stream);
/* d_reward (float) and d_reward64 (double) may each be NULL, as may d_obs, d_done and d_stats */
int pcgrl_smb_env_step(pcgrl_smb_env_handle h, const int32_t *d_actions, int32_t auto_reset, uint8_t *d_obs, float *d_reward,
                       double *d_reward64, uint8_t *d_done, int32_t *d_stats, void *stream);
int pcgrl_smb_env_observe(pcgrl_smb_env_handle h, uint8_t *d_obs, void *stream);
/* any output may be NULL.  d_grids uint8 [n][h][w], d_pos int32 [n][2], d_counters int32 [n][4] = iteration, changes, narrow's
 * scan counter, play-throughs run since the create, d_stats int32 [n][9], d_last_loss / d_ep_return double [n], d_iterations
 * int64 [n][2] = search iterations since the create, and the most one call spent */
int pcgrl_smb_env_get_state(pcgrl_smb_env_handle h, uint8_t *d_grids, int32_t *d_pos, int32_t *d_counters, int32_t *d_stats,
                            double *d_last_loss, double *d_ep_return, int64_t *d_iterations, void *stream);
/* the last finished episode of every env: return, length, final statistics, and how many have finished */
int pcgrl_smb_env_get_last_episode(pcgrl_smb_env_handle h, double *d_return, int32_t *d_length, int32_t *d_stats,
                                   int32_t *d_count, void *stream);
/* synchronises; PCGRL_EACTION for an action outside the space, PCGRL_EINVAL for a tile id above 6 in d_init_grids (or in the maps
 * of pcgrl_amd_smb_state.h's set call) and for an import index outside the batch (pcgrl_amd_smb_state.h) */
int pcgrl_smb_env_poll_error(pcgrl_smb_env_handle h);

#ifdef __cplusplus
}
#endif
#endif
