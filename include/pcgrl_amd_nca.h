/*
 * pcgrl_amd_nca.h -- the NCA level generator of libpcgrl_amd.so (companion of pcgrl_amd.h).
 *
 * The roll-out of the reference's default generator (--model NCA, --representation cellular; evo/models.py:62-116 and the
 * simulate loop of evo/evolve.py:944-1290) for G genomes x S seeds in one launch.  The net is
 *
 *   Conv2d(T, 32, 3, pad 1) -> relu -> Conv2d(32, 32, 1) -> relu -> Conv2d(32, T, 1) -> sigmoid
 *
 * on the one-hot map; the per-cell argmax is the whole next map; that repeats until the map stops changing or n_steps steps
 * are up, and only the final map is evaluated.  The dynamics are chaotic, so the arithmetic is this project's own statement,
 * restated in numpy in control_pcgrl_amd/nca.py (sigmoid32, stepped, generated); the kernel equals that bit for bit.  torch
 * sums in another order and its sigmoid differs in the last bit: no parity with torch is claimed beyond the recorded fixtures.
 * DESIGN.md section 38 has everything.
 *
 * Genome: a flat float32 vector in the order of the reference's get_init_weights / set_weights (evo/models.py:900-957):
 *
 *   l1.weight [32][T][3][3], l1.bias [32], l2.weight [32][32], l2.bias [32], l3.weight [T][32], l3.bias [T]
 *
 * that is P = 288 T + 32 + 1056 + 33 T floats (1730 for T = 2, 3656 for T = 8).  The hidden width is 32.  Auxiliary channels
 * (n_aux_chan > 0) and 3-D maps are not built.
 *
 * One step of one map (H x W, tiles 0..T-1), all in float32, every multiply and every add rounded on its own (no fused
 * multiply-add):
 *
 *   layer 1, per output channel o and cell:  acc = b1[o]; for c = 0..T-1, ky = 0..2, kx = 0..2 in that order: if the neighbour
 *            (y + ky - 1, x + kx - 1) is inside the map and holds tile c, acc = acc + w1[o][c][ky][kx]; taps outside the map
 *            are skipped; h1[o] = relu(acc)
 *   layer 2: acc = b2[o]; for c = 0..31: acc = acc + (w2[o][c] * h1[c]); h2[o] = relu(acc)
 *   layer 3: acc = b3[i]; for c = 0..31: acc = acc + (w3[i][c] * h2[c]); logit[i] = acc
 *   relu(a) = a < 0 ? 0 : a  (a NaN stays a NaN)
 *   next tile = the first index i at which s32(logit[i]) is largest
 *
 * s32 is the float32 sigmoid, defined with + - * / in double only:
 *
 *   a = min(|x|, 104);  z = -a;  k = rint(z * 1.4426950408889634)
 *   r = (z - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10
 *   p = 1/13!;  p = p * r + 1/n!  for n = 12 .. 0            (Horner, the degree-13 Taylor polynomial of exp)
 *   t = p * 2^k  (exact);  s = 1 / (1 + t) for x >= 0, else t / (1 + t);  s32 = (float)s
 *
 * It is monotone, 0.5 at 0, exactly 1 from about 17.33 on and exactly 0 from about -104 down, so saturated logits tie and the
 * first index wins -- which an argmax over the logits would not reproduce.
 *
 * Roll-out of (genome g, seed s): start from the init map; for n_step = 0, 1, ...: one step, change = any(next != map),
 * map = next; stop after the step at which !change or n_step >= n_steps - 1.  Outputs: the final map, that n_step (simulate's
 * time_penalty; the steps taken are n_step + 1) and, on request, the map after every step, rows past the end holding the final
 * map.
 *
 * Errors, per (g, s), with no host sync: an init tile >= T sets bit 0 (value 1) of the error word, a non-finite logit at any
 * cell of any step sets bit 1 (value 2).  In both cases the pair's output map and every one of its frames is its init map and
 * its n_step is -1; other pairs are undisturbed.
 *
 * pcgrl_nca_create checks its arguments before any HIP call (PCGRL_EINVAL: T outside 2..8, H or W outside 1..64, a null out)
 * and allocates the error word.  pcgrl_nca_generate checks its arguments (PCGRL_EINVAL) and then enqueues ONE kernel on
 * `stream`: no allocation, no host synchronisation, HIP-graph capturable.  pcgrl_nca_poll_error alone synchronises.  All data
 * pointers are device pointers; the outputs must not overlap the inputs.
 */
#ifndef PCGRL_AMD_NCA_H
#define PCGRL_AMD_NCA_H
#include <stddef.h>

#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCGRL_NCA_HIDDEN 32
#define PCGRL_NCA_MIN_TILES 2
#define PCGRL_NCA_MAX_TILES 8
#define PCGRL_NCA_MAX_SIDE 64
#define PCGRL_NCA_MAX_STEPS 1024
#define PCGRL_NCA_ERR_TILE 1
#define PCGRL_NCA_ERR_NONFINITE 2

int pcgrl_nca_create(int32_t n_tiles, int32_t height, int32_t width, int32_t device, void **out);
void pcgrl_nca_destroy(void *nca);

/* d_weights float [G][P]; d_init uint8 [S][H][W] (init_per_genome == 0: shared by all genomes) or [G][S][H][W]; n_steps in
 * 1..1024.  Outputs: d_levels uint8 [G][S][H][W], d_n_step int32 [G][S], d_frames uint8 [G][S][n_steps][H][W] or NULL.
 * G * S must be below 2^31. */
int pcgrl_nca_generate(void *nca, int32_t n_genomes, int32_t n_seeds, const float *d_weights, const uint8_t *d_init,
                       int32_t init_per_genome, int32_t n_steps, uint8_t *d_levels, int32_t *d_n_step, uint8_t *d_frames,
                       void *stream);

/* Reads and clears the error word; synchronises `stream`.  Negative on a HIP failure. */
int pcgrl_nca_poll_error(void *nca, void *stream);
const char *pcgrl_nca_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
