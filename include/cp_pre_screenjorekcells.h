/* cp_pre_screenjorekcells.h - C ABI of libcp_pre_screenjorekcells.so: the per-cell screens of cp_pre_screencells.h for the
 * reduced-MHD (JOREK) residuals of cp_pre_screenjorek.h - the question Marginal/JOREK_residuals_CP.py ends in: a quantile
 * per cell at ten alphas, and then, per alpha, which cells of the residual of every held-out prediction lie inside
 * [-qhat[k][cell], +qhat[k][cell]]:
 *   residual_continuity / residual_temperature          Marginal/JOREK_residuals_CP.py:210-243
 *   the per-cell sets at every alpha                    Marginal/JOREK_residuals_CP.py:297-311
 * Each entry is ONE streaming pass over the fields of a [B,T,X,Y] batch that evaluates the residual r in registers (the
 * functors of pre_residual_jorek_f32, unchanged: R is one more field, of which only the centre value is used) and reduces
 * it, per sample, to
 *   score[b]      = max over the counted cells of |r| / m                      (m == 1 without a modulation)
 *   count[k][b]   = number of counted cells with |r| <= hw,  hw = levels[k][cell]        without a modulation,
 *                                                            hw = fl(levels[k][cell] * m[cell])   with one
 * The residual is never written.  count is what pre_cov_levels_f32 counts on the stored residual with q_ld != 0, per sample.
 *
 * Conventions: this header defines no struct of its own.  Both entries take the argument list of their twin in
 * cp_pre_screenjorek.h with the set descriptor swapped for the per-cell one of cp_pre_screencells.h:
 *   - eq: 0 continuity (fields rho, phi; fields[2] is not read), 1 temperature (rho, phi, T);
 *   - fields: the three views of the [B,T,X,Y] batch, in the entry's layout;
 *   - Rb: the radius as a view of the fields' shape that repeats its row along Y - Ny-fastest: strides (0, 0, 0, 1) over Y
 *     floats; Nt-fastest: strides (sB, sT, sX, sY) = (0, 1, 0, T) over a [Y][T] array.  It is checked like a field;
 *   - K_t, K_R, K_Z, K_RR, K_ZZ: host, dense 3x3x3 on (T, X, Y); coef: host, the four scalars a0..a3 of
 *     pre_residual_jorek_f32 (continuity: (1, 1, 2, D), or with norms (dx dy, dt dy, 2 dt dx, D); temperature:
 *     (2 gamma, 0, 0, K));
 *   - s: pre_screencells_t for the Ny-fastest entry, pre_screencellsflat_t for the flat one, with that header's layouts of
 *     the level fields and the modulation, its rim and its non-finite contract (a NaN level or a NaN residual puts the cell
 *     outside at that level, a negative level outside, +inf inside for every non-NaN residual);
 *   - B, T, X, Y: the extents of a view; flags: the twin's (0 for the flat entry; neither entry reads halo rows of x);
 *   - stream: the hipStream_t all work is enqueued on;
 *   - the tap structure is chosen as pre_residual_jorek_f32 chooses it: the reference's construction, the y-fixed one, or the
 *     general star when D_RR does not fit D_R's tap structure or D_ZZ that of D_Z.  Every tap structure of both equations is
 *     built in both forms: no instantiation has scratch;
 *   - block order: the samples in groups of pre_screenjorekcells_sample_group(), the sample of a group the fastest block
 *     index (cp_pre_screencells.h).  Speed only.
 *
 * Checks, in this order, before any launch:
 *   - PRE_E_NULL for a null fields, Rb, kernel or coef;
 *   - PRE_E_RANGE for eq outside [0, 1];
 *   - everything the twin's descriptor checks (cp_pre_screen.h / cp_pre_screenflat.h): PRE_E_NULL for a null s, levels,
 *     score, count or view pointer, an empty extent or count_ld < B; PRE_E_RANGE for nk outside
 *     [1, PRE_SCREEN_MAX_LEVELS] or a negative crop; PRE_E_UNSUPPORTED for a layout the form does not take (R's view
 *     included) and the flags it does not take; PRE_E_SHAPE as in the two headers;
 *   - the level strides as cp_pre_screencells.h states them: PRE_E_SHAPE for a negative one, PRE_E_UNSUPPORTED for level
 *     fields of an Nt-fastest entry that are not in the fields' in-plane layout (lT == 1, lY == T);
 *   - PRE_E_UNSUPPORTED for operator weight off the 7-point star.
 * Nothing allocates, nothing synchronises.
 */
#ifndef CP_PRE_SCREENJOREKCELLS_H
#define CP_PRE_SCREENJOREKCELLS_H

#include <stdint.h>

#include "cp_pre_screencells.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SCREENJOREKCELLS_ABI_VERSION 1
int pre_screenjorekcells_abi_version(void);   /* == PRE_SCREENJOREKCELLS_ABI_VERSION */
int pre_screenjorekcells_sample_group(void);  /* samples per group of the block order (>= 1), a constant of the build */

/* Ny-fastest fields (every view, Rb, the modulation and the level fields with unit stride on Y, Y % 4 == 0): r = equation
 * `eq` of pre_residual_jorek_f32, Marginal/JOREK_residuals_CP.py:210-243, screened as Marginal/JOREK_residuals_CP.py:297-311
 * does at every alpha. */
int pre_screenjorekcells_f32(int eq, const pre_field_t fields[3], const pre_field_t *Rb,
                             const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                             const float coef[4], const pre_screencells_t *s,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* Nt-fastest fields - the layout the script holds: vars[BS,F,Nx,Ny,Nt] dense, each field its permute(0,3,1,2) view (sT == 1,
 * sY == T; Rb, the modulation and the level fields likewise): r = equation `eq` of pre_residual_jorek_f32,
 * Marginal/JOREK_residuals_CP.py:210-243, screened as Marginal/JOREK_residuals_CP.py:297-311 does at every alpha. */
int pre_screenjorekcells_flat_f32(int eq, const pre_field_t fields[3], const pre_field_t *Rb,
                                  const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                                  const float coef[4], const pre_screencellsflat_t *s,
                                  int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_SCREENJOREKCELLS_H */
