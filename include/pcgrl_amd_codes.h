/*
 * pcgrl_amd_codes.h -- the tile-code observation form of libpcgrl_amd.so (companion of pcgrl_amd.h).
 *
 * pcgrl_observe and the observation outputs of pcgrl_step / pcgrl_rollout / pcgrl_update / pcgrl_step_ready write the
 * reference's one-hot image (wrappers.py:407-437 Cropped -> :232-257 OneHotEncoding -> :140-150 ToImage).  The code form is
 * the same stack with OneHotEncoding left out: one byte per cell and plane, channel-last uint8, a ninth (zelda) / a third
 * (binary) of the bytes.  A policy expands it in its first layer; one_hot(codes[..., 0], C) ++ codes[..., 1:] is the one-hot
 * observation bit for bit.
 *
 *   config            codes shape              plane 0                                   extra plane          C
 *   narrow / turtle   [N][OH][OW][P]           0 = outside the map, 1 + tile inside       static mask (0        n_tiles + 1
 *                     P = 1 + static_tiles                                                outside), optional
 *   wide              [N][H][W][1]             tile                                       --                   n_tiles
 *   3-D maze          [N][o0][o1][o2][1]       0 out of bounds, 1 AIR, 2 DIRT, 3 path     --                   4
 *
 * The form is a property of the caller's buffers, not of the engine: the config, the state, pcgrl_state_bytes and
 * checkpoints are the same in either form.  Every entry point below only enqueues kernels on `stream` (HIP-graph capturable)
 * and checks its handle and pointers before any HIP call (PCGRL_EINVAL).
 */
#ifndef PCGRL_AMD_CODES_H
#define PCGRL_AMD_CODES_H
#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the codes shape of one env (ndim 3 for 2-D problems, 4 for the 3-D maze) and its byte count */
int pcgrl_codes_shape(pcgrl_handle h, int32_t shape_out[4], int32_t *ndim_out);
int64_t pcgrl_codes_bytes(pcgrl_handle h);

/* The codes of the current state of every env: what pcgrl_observe shows, as codes.  2-D problems (one launch, from the tile
 * planes); PCGRL_EUNSUPPORTED for the 3-D maze, whose observation also shows the overlay of the last statistics update:
 * pcgrl_observe into a one-hot buffer, then pcgrl_onehot_to_codes.  d_codes: uint8 [N][pcgrl_codes_bytes], any alignment.
 * After pcgrl_step / pcgrl_step_ex / pcgrl_update / pcgrl_reset with d_obs == NULL this is the observation those calls
 * would have written (the 2-D observation is a function of the state after the call). */
int pcgrl_observe_codes(pcgrl_handle h, uint8_t *d_codes, void *stream);

/* n_rows one-hot observations (pcgrl_obs_bytes each, as written by any entry point of pcgrl_amd.h) -> n_rows rows of codes
 * (pcgrl_codes_bytes each).  For observations that are not a function of the state after the call: the 3-D maze, rollouts
 * that return every step's observation.  d_onehot and d_codes must not overlap. */
int pcgrl_onehot_to_codes(pcgrl_handle h, const uint8_t *d_onehot, int64_t n_rows, uint8_t *d_codes, void *stream);

/* pcgrl_step_ready with codes.  d_scratch (uint8 [N][pcgrl_obs_bytes], caller-owned) is the env's PERSISTENT one-hot
 * observation buffer: pcgrl_step_ready writes the rows it writes there and leaves the others as they are (a busy env's row,
 * as pcgrl_step_ready leaves it), then every row of d_scratch is converted into d_codes.  So the caller keeps d_scratch where
 * it would keep a one-hot observation buffer -- pcgrl_reset / pcgrl_observe write it too -- and d_codes is always the code
 * form of that buffer. */
int pcgrl_step_ready_codes(pcgrl_handle h, const int32_t *d_actions, int32_t auto_reset, uint8_t *d_scratch, uint8_t *d_codes,
                           float *d_reward, uint8_t *d_done, int32_t *d_stats, uint8_t *d_status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
