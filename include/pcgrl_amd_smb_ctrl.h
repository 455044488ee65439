/*
 * pcgrl_amd_smb_ctrl.h -- controllable generation for the Super Mario Bros environments of pcgrl_amd_smb_env.h: what
 * ControlWrapper(ctrl_metrics=cfg.controls) of the reference adds to SMBCtrlProblem (control_wrappers.py:27-121, :167-214,
 * :318-345), with the device contract the engine of pcgrl_amd.h has for its problems.
 *
 *   targets   every env holds active targets for all nine statistics (the zero-loss interval lo..hi, both ends included); they
 *             start as the config's.  pcgrl_smb_ctrl_queue only queues: the queue is applied at the env's next reset (explicit or
 *             automatic), before the new level's loss is taken, and replaces the targets of the controls it names only.  A second
 *             call before the reset replaces the first, as set_trgs does.  The step that ends an episode is rewarded against
 *             the old targets.
 *   loss      -(distance of the statistic to lo..hi) * weight, the terms in the statistics' order, each rounded to double and
 *             then added (no fused multiply-add); reward = loss - last_loss in double.  Targets need not be integers.
 *   ctrl_obs  float32 [n_envs][2 * n_ctrl]: per control j (observed target value / range, statistic / range), range the
 *             |cond_bounds| given at the attach.  The observed value of a (lo, hi) tuple is the caller's -- the reference shows
 *             the midpoint of the raw tuple, not of the zero-loss interval.  The row is written by every launch that writes the
 *             env's statistics row (reset, step, ready step, rollout: after its last step, state set) into the buffer given at
 *             the attach.
 *   resample  with resampling enabled every reset draws each control's target uniformly in [lo_j, hi_j) from the env's own
 *             counter-based stream -- trg_resampled of pcgrl_set_target_resampling (pcgrl_amd.h), with the env's draw counter,
 *             which advances at every reset of that env -- and the draw replaces whatever was queued.
 *   state     the image of pcgrl_amd_smb_state.h gains a section with the per-env control records (active and queued targets,
 *             flag word with the draw counter); its header covers the control list and ranges, so an image with controls and an
 *             env without refuse each other.  The resampling switch, seed and bounds are run-time state, not in the image.
 *
 * Every call checks its arguments before any HIP call and then -- the attach apart, which allocates and synchronises -- enqueues
 * one kernel on `stream`: no allocation, no synchronisation, HIP-graph capturable.
 */
#ifndef PCGRL_AMD_SMB_CTRL_H
#define PCGRL_AMD_SMB_CTRL_H
#include "pcgrl_amd_smb_env.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Turns the handle controllable: once, before its first reset (PCGRL_EINVAL after one, after a state set or import, or twice).
 * ctrl_idx [n_ctrl]: the statistics controlled, no duplicates; ctrl_range [n_ctrl] > 0; shown [n_ctrl]: the value the control
 * observation shows for the config's static target; d_ctrl_obs float [n_envs][2 * n_ctrl] on the device, or NULL for none. */
int pcgrl_smb_ctrl_attach(pcgrl_smb_env_handle h, int32_t n_ctrl, const int32_t *ctrl_idx, const double *ctrl_range,
                          const double *shown, float *d_ctrl_obs);
/* the number of controls; 0 for a handle without, -1 for a null handle */
int32_t pcgrl_smb_ctrl_count(pcgrl_smb_env_handle h);
/* Queues targets for the envs of d_mask (uint8 [n_envs], NULL = all).  named [n_named] (host): positions in the control list,
 * no duplicates; d_lo, d_hi, d_shown double [n_envs][n_named] on the device: the zero-loss interval and the observed value. */
int pcgrl_smb_ctrl_queue(pcgrl_smb_env_handle h, const uint8_t *d_mask, int32_t n_named, const int32_t *named,
                         const double *d_lo, const double *d_hi, const double *d_shown, void *stream);
/* the control observation of the committed state, into d_ctrl_obs or (NULL) into the attached buffer */
int pcgrl_smb_ctrl_observe(pcgrl_smb_env_handle h, float *d_ctrl_obs, void *stream);
/* lo, hi [n_ctrl] (host): the bounds of the draw; they may be NULL when enable is 0.  Takes effect in stream order. */
int pcgrl_smb_ctrl_set_resampling(pcgrl_smb_env_handle h, int32_t enable, uint64_t seed, const double *lo, const double *hi,
                                  void *stream);
/* for tests; any output may be NULL.  d_active double [n_envs][9][2] = lo, hi per statistic; d_shown double [n_envs][9] and
 * d_queued double [n_envs][9][3] = lo, hi, observed value, both per control (rows n_ctrl.. unused); d_flags int32 [n_envs][2] =
 * the flag word (bit 0: targets are queued, bits 1..: the draw counter) and the set of controls the queue names */
int pcgrl_smb_ctrl_get(pcgrl_smb_env_handle h, double *d_active, double *d_shown, double *d_queued, int32_t *d_flags,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif
