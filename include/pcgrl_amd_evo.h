/*
 * pcgrl_amd_evo.h -- NCA evolution on the device (companion of pcgrl_amd_archive.h and pcgrl_amd_nca.h).
 *
 * The reference's default evolution (`--model NCA --representation cellular`) evolves the weights of the NCA, not maps: the
 * child of a genome is w += randn_like(w) * sqrt(step_size) (evo/models.py:31-38), and a candidate is scored by what simulate
 * folds over its S levels (evo/evolve.py:1125-1154, :1209-1244).  This header adds what the loop
 *
 *   ask -> pcgrl_nca_generate -> evaluate -> behaviour -> aggregate -> add
 *
 * lacked to stay on one stream: archives whose elite is a genome, Gaussian children with stated arithmetic, and the fold over
 * seeds.  DESIGN.md section 42 has everything; control_pcgrl_amd/evo.py has the numpy twins, which the kernels equal bit for
 * bit.  torch's randn stream is not reproduced.
 *
 * 1. Genome archives.  pcgrl_archive_create_genomes makes an archive of pcgrl_amd_archive.h's handle type whose per-cell
 * payload is a float32 [P] row (P in 1..16384, rows padded to 16 bytes) where a map archive has its map.  cells x row bytes
 * above 2^32 is refused with PCGRL_EINVAL before any HIP call.  pcgrl_archive_add, _cells, _stats, _elites, _export, _import,
 * _state_bytes and _poll_error serve it, taking and returning the payload rows (4 P bytes each, any 4-byte alignment) where
 * they say d_maps; placement, insertion order, statuses, counts and error bits are exactly those of pcgrl_amd_archive.h.  The
 * image has the same sections; its header carries L = 4 P and T = 0.  A genome image and a map archive refuse each other
 * before anything is overwritten, in both directions; a map archive's image is byte for byte what it was.  pcgrl_archive_ask
 * on a genome archive returns PCGRL_EINVAL and names pcgrl_archive_ask_genomes; the two calls below on a map archive return
 * PCGRL_EINVAL and name pcgrl_archive_ask.
 *
 * 2. The normal draw.  For element k of child c, with base and mix() of pcgrl_amd_archive.h, in 64-bit wrapping arithmetic:
 *
 *   gb = mix(base ^ (c * 0xd1b54a32d192ed03 + 3 * 0x8cb92ba72f3d8dd7))
 *   q  = mix(gb + (k + 1) * 0x9e3779b97f4a7c15)
 *   u  = ((q >> 11) + 0.5) * 2^-53                      (never 0 or 1)
 *   z  = ppnd(u)
 *
 * ppnd is Wichura's AS241 PPND16 in double: the three rational functions by Horner, numerator and denominator apart, then
 * one division; the regions are |u - 0.5| <= 0.425, r <= 5 and r > 5 with r = sqrt(-log64(min(u, 1 - u))).  log64 is this
 * project's: x = m 2^e by the bits with m in [sqrt(1/2), sqrt(2)), f = (m - 1) / (m + 1), p the Horner polynomial in f^2 with
 * the coefficients 1/25, 1/23, ..., 1/1, and log64 = e ln2_hi + ((2 f) p + e ln2_lo) with ln2_hi = 6.93147180369123816490e-01,
 * ln2_lo = 1.90821492927058770002e-10.  Only + - * /, correctly rounded sqrt, comparisons and bit operations are used, each
 * rounded on its own: no fused multiply-add, no library log / exp / sin / cos.
 *
 * 3. Children.  Child c of pcgrl_archive_ask_genomes draws its parent exactly as pcgrl_archive_ask does (same formula, same
 * salt) and is  child[k] = parent[k] + ((float)z * sigma):  one float32 multiply, then one float32 add.  sigma is a finite
 * float >= 0 (the reference's is sqrt(0.01)); sigma == 0 returns the parents' bits (the add is skipped).  On an empty archive
 * error bit 1 is set and nothing is written.  pcgrl_archive_sample_genomes is the same draw without a parent,
 * mean[k] + (float)z * sigma with mean zero when d_mean is NULL: the first generation's ask around an initial genome; it
 * works on an empty archive.  Both advance the device's draw counter by one (ask_genomes only when it drew), allocate
 * nothing, do no host sync and can be captured.
 *
 * 4. pcgrl_evo_aggregate: simulate's fold over the S levels of each of G genomes.  Inputs d_objective double [G][S] (the
 * per-level objective, for an evaluator -loss), d_behaviours double [G][S][D], d_n_step int32 [G][S]; G >= 1, S in 1..128, D in
 * 1..4.  Outputs per genome:
 *
 *   behaviours        double [G][D]  the mean of the S values (numpy's np.mean)
 *   objective         double [G]     (weight * acc) / S, acc the sequential sum in seed order from 0
 *   time_penalty      int32 [G]      -(sum of n_step)
 *   variance_penalty  double [G]     -(std_0 + ... + std_{D-1}) / D, std_j = sqrt(sum((x - mean) * (x - mean)) / S)
 *   valid             uint8 [G]      0 if any n_step of the genome is negative (a pair the generator refused)
 *
 * An invalid genome's objective and behaviours are NaN, so pcgrl_archive_add refuses it with status 3.  Sums other than acc
 * are numpy's: below 8 elements sequential; from 8 to 128 eight accumulators take the elements of stride 8 over the first
 * S - S % 8 elements, are combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), and the remainder is added in order.
 *
 * Every call checks its arguments (PCGRL_EINVAL) and then only enqueues kernels on `stream`.  pcgrl_archive_last_error has
 * the message.
 */
#ifndef PCGRL_AMD_EVO_H
#define PCGRL_AMD_EVO_H
#include <stddef.h>

#include "pcgrl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCGRL_EVO_MAX_PARAMS 16384
#define PCGRL_EVO_MAX_SEEDS 128
#define PCGRL_EVO_MAX_BEHAVIOURS 4

int pcgrl_archive_create_genomes(int32_t n_axes, const int32_t *dims, const double *lo, const double *hi, int32_t n_params,
                                 int32_t device, void **out);

/* n children: d_out float [n][P] (any 4-byte alignment), d_out_parent_cell int32 [n] (may be NULL). */
int pcgrl_archive_ask_genomes(void *archive, int32_t n, uint64_t seed, float sigma, float *d_out, int32_t *d_out_parent_cell,
                              void *stream);

/* n draws around d_mean float [P] (NULL: zero): d_out float [n][P]. */
int pcgrl_archive_sample_genomes(void *archive, int32_t n, uint64_t seed, float sigma, const float *d_mean, float *d_out,
                                 void *stream);

int pcgrl_evo_aggregate(int32_t n_genomes, int32_t n_seeds, int32_t n_behaviours, double weight, const double *d_objective,
                        const double *d_behaviours, const int32_t *d_n_step, double *d_out_behaviours, double *d_out_objective,
                        int32_t *d_out_time_penalty, double *d_out_variance_penalty, uint8_t *d_out_valid, void *stream);

#ifdef __cplusplus
}
#endif
#endif
