/*
 * pcgrl_amd_smb_vector.h -- the float32 hand-out of the Super Mario Bros environments of pcgrl_amd_smb_env.h: the observation
 * in the form RLlib's Box declares, written once by a kernel of its own.
 *
 *   image     float32 [n_envs][oh][ow][C], C = 2K + 8 with K = pcgrl_smb_ctrl_count(h) (0 without controls).  Channels
 *             0 .. 2K-1 hold the env's control observation (pcgrl_amd_smb_ctrl.h: per control target / range, statistic / range)
 *             broadcast over the window -- the planes come first, as ControlWrapper puts them (control_wrappers.py:189-214);
 *             channel 2K is 1.0 outside the map and channel 2K + 1 + tile is 1.0 inside; everything else is 0.0.  The window is
 *             centred on the position as pcgrl_smb_env_observe's is (row pos - oh / 2 is the first).
 *   inputs    the committed state of the handle -- maps and positions -- and, with controls, the control observation in the
 *             buffer given to pcgrl_smb_ctrl_attach, which reset / step have written.  A controllable handle attached with a
 *             NULL control observation is refused (PCGRL_EINVAL).
 *   order     the call shows the state of the reset / step it is ordered after: enqueue it on the same stream, after that call.
 *   out       device memory or host-mapped pinned memory, 8-byte aligned (16 lets every env of every shape start on whole
 *             16-byte stores; on 8 the kernel stores a 2-float head and tail around them).
 *   async     a handle in asynchronous mode (pcgrl_smb_ready_set_budget with a positive budget) is refused with
 *             PCGRL_EUNSUPPORTED: a busy env's committed state is not the state of the step in flight.
 *
 * pcgrl_smb_env_observe_f32 checks its arguments before any HIP call -- PCGRL_EINVAL for a null handle, a null `out` or an `out`
 * that is not 8-byte aligned -- and then enqueues one kernel on `stream`: no allocation, no synchronisation, HIP-graph
 * capturable.
 *
 * The statistics of the committed state are pcgrl_smb_env_get_state's d_stats (every other output NULL); like
 * pcgrl_smb_env_step and pcgrl_smb_env_reset it checks alignment only, so its outputs may be host-mapped pinned memory too.
 */
#ifndef PCGRL_AMD_SMB_VECTOR_H
#define PCGRL_AMD_SMB_VECTOR_H
#include "pcgrl_amd_smb_ctrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of one env's float32 image: oh * ow * (2K + 8) * 4; -1 on a null handle */
int64_t pcgrl_smb_env_obs_f32_bytes(pcgrl_smb_env_handle h);
int pcgrl_smb_env_observe_f32(pcgrl_smb_env_handle h, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
