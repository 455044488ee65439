/*
 * pcgrl_amd_nca3d.h -- the 3-D NCA level generator of libpcgrl_amd.so, plain and holey (companion of pcgrl_amd.h and
 * pcgrl_amd_nca.h).
 *
 * The roll-out of the reference's --model NCA3D (evo/models.py:180-219) under --representation cellular3D (plain) and
 * cellular3Dholey (holey; evo/evolve.py:347-361, :1003-1106) for G genomes x S seeds in one launch.  The net is
 *
 *   Conv3d(T, 32, 3, pad 1) -> relu -> Conv3d(32, 32, 1) -> relu -> Conv3d(32, T, 1) -> sigmoid
 *
 * on the one-hot map; the per-cell first argmax is the whole next map; that repeats until the map stops changing or n_steps
 * steps are up (n_step has simulate's meaning, as in pcgrl_amd_nca.h).  As there, the arithmetic is this project's own
 * statement, restated in numpy in control_pcgrl_amd/nca3d.py (stepped, generated); the kernel equals that bit for bit, and no
 * parity with torch is claimed beyond the recorded fixtures.  DESIGN.md section 44 has everything.
 *
 * Maps are uint8 [D0][D1][D2], each axis 3..16, in the axis order of pcgrl_amd_mc3d_holey.h (Z, Y, X); kernel index
 * (k0, k1, k2) runs along those axes in that order.  T is in 2..8.
 *
 * Genome: a flat float32 vector in the order of the reference's get_init_weights:
 *
 *   l1.weight [32][T][3][3][3], l1.bias [32], l2.weight [32][32], l2.bias [32], l3.weight [T][32], l3.bias [T]
 *
 * that is P = 864 T + 32 + 1056 + 33 T floats (2882 for T = 2, 5573 for T = 5, 8264 for T = 8).  Auxiliary channels are not
 * built.
 *
 * Two modes, one kernel.  Both read an IMAGE: the map inside a one-cell ring, [D0 + 2][D1 + 2][D2 + 2].
 *   plain  (d_holes == NULL) the ring holds no tile: a tap on it adds nothing (zero padding).
 *   holey  the ring holds border_tile, except the four cells of the two holes, which hold empty_tile: d_holes gives the foot
 *          cells (z, y, x) of the entrance and the exit in image (bordered) coordinates, and each head is at z + 1, as
 *          HoleyRepresentation3D.dig_holes sets them.  Only the interior is updated (cut_border_action_3d), the change test is
 *          on the interior, and border and holes never change; nothing beyond the ring is ever read.
 *
 * One step, all in float32, every multiply and every add rounded on its own (no fused multiply-add):
 *
 *   layer 1, per output channel o and interior cell (z, y, x):  acc = b1[o]; for k0 = 0..2, k1 = 0..2, k2 = 0..2 in that
 *            order: if the image cell (z + k0 - 1, y + k1 - 1, x + k2 - 1) holds a tile c, acc = acc + w1[o][c][k0][k1][k2];
 *            h1[o] = relu(acc).
 *            THE ORDER IS BY TAP, NOT BY TILE.  The 2-D generator sums by (tile, ky, kx), which costs it a sort of nine keys
 *            per cell; with 27 taps that sort would cost more than the layer, and the order is this project's choice either
 *            way, because torch's is its own.  A 3-D genome's logits are therefore not the 2-D rule along one more axis.
 *   layer 2: acc = b2[o]; for c = 0..31: acc = acc + (w2[o][c] * h1[c]); h2[o] = relu(acc)
 *   layer 3: acc = b3[i]; for c = 0..31: acc = acc + (w3[i][c] * h2[c]); logit[i] = acc
 *   relu(a) = a < 0 ? 0 : a  (a NaN stays a NaN)
 *   next tile = the first index i at which s32(logit[i]) is largest, s32 being the float32 sigmoid of pcgrl_amd_nca.h
 *
 * Roll-out and outputs are those of pcgrl_amd_nca.h, on the interior: the final map, n_step and, on request, the map after
 * every step, rows past the end holding the final map.
 *
 * Errors, per (g, s), with no host sync: an init tile >= T sets bit 0 (value 1) of the error word, a non-finite logit at any
 * cell of any step bit 1 (value 2), a hole that the rule of pcgrl_amd_mc3d_holey.h rejects (the foot on one of the four side
 * faces, off the edges, 1 <= z <= D0 - 1) bit 2 (value 4).  In every case the pair's output map and every one of its frames is
 * its init map and its n_step is -1; other pairs are undisturbed.
 *
 * Kernel: one workgroup per (g, s); passes = ceil(cells / 256) and ceil(cells / passes) lanes rounded up to 64 (7 x 7 x 7 runs
 * two passes of 192 lanes).  pcgrl_nca3d_create checks its arguments before any HIP call (PCGRL_EINVAL: T outside 2..8, an axis
 * outside 3..16, a null out) and allocates the error word.  pcgrl_nca3d_generate checks its arguments (PCGRL_EINVAL; with holes,
 * border_tile and empty_tile must be below T) and then enqueues ONE kernel on `stream`: no allocation, no host synchronisation,
 * HIP-graph capturable.  pcgrl_nca3d_poll_error alone synchronises.  All data pointers are device pointers; the outputs must not
 * overlap the inputs.
 */
#ifndef PCGRL_AMD_NCA3D_H
#define PCGRL_AMD_NCA3D_H
#include <stddef.h>

#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCGRL_NCA3D_MIN_AXIS 3
#define PCGRL_NCA3D_MAX_AXIS 16
#define PCGRL_NCA3D_ERR_TILE 1
#define PCGRL_NCA3D_ERR_NONFINITE 2
#define PCGRL_NCA3D_ERR_HOLE 4

int pcgrl_nca3d_create(int32_t n_tiles, int32_t d0, int32_t d1, int32_t d2, int32_t device, void **out);
void pcgrl_nca3d_destroy(void *nca3d);

/* d_weights float [G][P]; d_init uint8 [S][D0][D1][D2] (init_per_genome == 0: shared by all genomes) or [G][S][D0][D1][D2];
 * d_holes NULL (plain) or int32 [2][3] (holes_per_seed == 0: all seeds) or [S][2][3]; n_steps in 1..1024.  Outputs: d_levels
 * uint8 [G][S][D0][D1][D2], d_n_step int32 [G][S], d_frames uint8 [G][S][n_steps][D0][D1][D2] or NULL.  G * S must be below
 * 2^31. */
int pcgrl_nca3d_generate(void *nca3d, int32_t n_genomes, int32_t n_seeds, const float *d_weights, const uint8_t *d_init,
                         int32_t init_per_genome, const int32_t *d_holes, int32_t holes_per_seed, int32_t border_tile,
                         int32_t empty_tile, int32_t n_steps, uint8_t *d_levels, int32_t *d_n_step, uint8_t *d_frames,
                         void *stream);

/* Reads and clears the error word; synchronises `stream`.  Negative on a HIP failure. */
int pcgrl_nca3d_poll_error(void *nca3d, void *stream);
const char *pcgrl_nca3d_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
