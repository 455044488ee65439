/*
 * pcgrl_amd_smb_state.h -- checkpoint and restore of the Super Mario Bros environments of pcgrl_amd_smb_env.h, with or without
 * the solver budget of pcgrl_amd_smb_ready.h: what pcgrl_export_state / pcgrl_import_state / pcgrl_set_state /
 * pcgrl_get_rng_state of pcgrl_amd.h are to the 2-D engine (the reference pickles the whole env: envs/pcgrl_env.py:102-112).
 *
 * The image.  pcgrl_smb_state_bytes = a 256-byte header plus, per env, the stored map row (H * W rounded up to 16 bytes), the
 * env's record (144 bytes: position, counters, the nine statistics, last_loss, the running and the last episode's return,
 * lengths and statistics, searches and the iteration counters), both PCG64 streams as the ten words pcgrl_get_rng_state of
 * pcgrl_amd.h documents (the kept 32-bit half is always empty here: an SMB env draws doubles only) and two int32: the env's ready
 * mode (0 idle, 1 a pending step, 2 pending statistics) and the pending action.  Each of the four is one section, contiguous over
 * the envs.  The header holds a magic number, the batch size, the per-env layout and a fingerprint of every create-time field of
 * pcgrl_smb_env_config, the batch size, the library version and the layout; the solver budget is not part of it.
 *
 * A parked search is not in the image -- neither the loop's words nor the visited set nor the workspace slot -- and neither
 * are the error word and the budget.  An imported busy env stays busy, with the same pending action or the same fresh level,
 * and its search STARTS OVER: the first launch after the import plays it from iteration 0.  A search is a function of the map
 * and solver_power alone, and an exported busy env's iteration total excludes what its parked search had spent, so every
 * emitted transition and every counter but the most-per-launch one equals the uninterrupted run's; only the launch at which
 * the env emits is later.
 *
 * Every entry point returns 0 or a PCGRL_E* code with the message in pcgrl_last_error(), refuses a null handle with PCGRL_EINVAL
 * before any HIP call, and is asynchronous on `stream` -- but for the one wait of pcgrl_smb_state_import.  Export, set and the
 * stream calls are one kernel each, read nothing on the host and are HIP-graph capturable.  Buffers are 16-byte aligned.
 */
#ifndef PCGRL_AMD_SMB_STATE_H
#define PCGRL_AMD_SMB_STATE_H
#include "pcgrl_amd.h"
#include "pcgrl_amd_smb_env.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of an image of this env; -1 for a null handle */
int64_t pcgrl_smb_state_bytes(pcgrl_smb_env_handle h);

/* d_buf uint8 [pcgrl_smb_state_bytes]: the state at the moment the launch runs (a captured export writes the state of every
 * replay's moment).  The header is copied from pinned memory the library owns.  Without a budget every mode is idle. */
int pcgrl_smb_state_export(pcgrl_smb_env_handle h, uint8_t *d_buf, void *stream);

/* Into an env created with the same config and batch size.  d_mask uint8 [n_envs] (NULL = all) selects the envs that are
 * overwritten, d_index int32 [n_envs] (NULL = identity) names the image row each of them takes; an entry outside 0..n_envs-1
 * overwrites nothing and sets an error bit that pcgrl_smb_env_poll_error reports.  The header is checked on the host after one
 * wait for `stream`; any other image -- another shape, representation, window, limits, solver_power, weights or targets, batch
 * size or library version, or a damaged header -- is refused with PCGRL_EINVAL before anything is overwritten.
 * Modes: an env without a budget cannot finish a parked search, so an image that would give it a busy row (under the mask and
 * the index) is refused with PCGRL_EUNSUPPORTED, which names the count of such rows, and nothing is overwritten; an image of
 * an env without a budget imports into a budgeted one, everything idle.  The park records of the overwritten envs are cleared
 * (their searches are abandoned, as a masked reset abandons them); every other env keeps what it has parked. */
int pcgrl_smb_state_import(pcgrl_smb_env_handle h, const uint8_t *d_mask, const int32_t *d_index, const uint8_t *d_buf,
                           void *stream);

/* The portable form, the mirror of pcgrl_smb_env_get_state's first fields, for the envs of d_mask (NULL = all): d_grids uint8
 * [n_envs][H * W], d_pos int32 [n_envs][2] (NULL = the origin; clamped to the map), d_counters int32 [n_envs][4] = iteration,
 * changes, n_step, searches and d_ep_return double [n_envs] (either NULL = zero).  The nine statistics and last_loss are
 * recomputed from the map by the level's evaluation, whose iterations are counted; under a budget the evaluation may leave the
 * env busy with pending statistics (`searches` then shows one less until they arrive).  A tile id above 6 is read as empty and
 * sets the error bit pcgrl_smb_env_reset sets.  The last finished episode and the RNG streams are left alone. */
int pcgrl_smb_state_set(pcgrl_smb_env_handle h, const uint8_t *d_mask, const uint8_t *d_grids, const int32_t *d_pos,
                        const int32_t *d_counters, const double *d_ep_return, void *stream);

/* d_rng uint64 [n_envs][10] in the layout of pcgrl_get_rng_state: rep {state hi, lo, inc hi, lo}, prob {...}, 0, 0 */
int pcgrl_smb_state_get_rng(pcgrl_smb_env_handle h, uint64_t *d_rng, void *stream);
int pcgrl_smb_state_set_rng(pcgrl_smb_env_handle h, const uint8_t *d_mask, const uint64_t *d_rng, void *stream);

#ifdef __cplusplus
}
#endif
#endif
