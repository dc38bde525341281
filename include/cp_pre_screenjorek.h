/* cp_pre_screenjorek.h - C ABI of libcp_pre_screenjorek.so: the calibrated-set screens of cp_pre_screen.h (Ny-fastest
 * fields) and cp_pre_screenflat.h (Nt-fastest fields) for the reduced-MHD (JOREK) residuals - the question
 * Joint/JOREK_residuals_CP.py ends in:
 *   residual_continuity / residual_temperature          Joint/JOREK_residuals_CP.py:210-243
 *   ncf_metric_joint, then the coverage of the set      Joint/JOREK_residuals_CP.py:297-308
 * Each entry is ONE streaming pass over the fields of a [B,T,X,Y] batch that evaluates the residual r in registers (the
 * functors of pre_residual_jorek_f32, unchanged: R is one more field, of which only the centre value is used) and reduces
 * it, per sample, to
 *   score[b]      = max over the counted cells of |r| / m
 *   count[k][b]   = number of counted cells with |r| <= q[k] * m   (k < nk <= PRE_SCREEN_MAX_LEVELS)
 * The residual is never written.
 *
 * Both entries take the argument list of pre_residual_jorek_f32 with the set descriptor in place of `out`:
 *   - eq: 0 continuity (fields rho, phi; fields[2] is not read), 1 temperature (rho, phi, T);
 *   - Rb: the radius as a view of the fields' shape that repeats its row along Y - Ny-fastest: strides (0, 0, 0, 1) over Y
 *     floats; Nt-fastest: strides (sB, sT, sX, sY) = (0, 1, 0, T) over a [Y][T] array.  It is checked like a field;
 *   - K_t, K_R, K_Z, K_RR, K_ZZ: host, dense 3x3x3 on (T, X, Y); coef: host, the four scalars a0..a3 of
 *     pre_residual_jorek_f32 (continuity: (1, 1, 2, D); temperature: (2 gamma, 0, 0, K));
 *   - the tap structure is chosen as pre_residual_jorek_f32 chooses it: the reference's construction, the y-fixed one, or the
 *     general star when D_RR does not fit D_R's tap structure or D_ZZ that of D_Z.  Every tap structure of both equations is
 *     built in both forms: no instantiation has scratch.  (One that had would not be built: its entry would return
 *     PRE_E_UNSUPPORTED for that mode, as pre_screen_mhd_f32 does for the general star of the energy equation.)
 *
 * Everything else - accumulation, the non-finite contract, hw = q[k] * m, `q` on the device, the accepted layouts, the
 * flags - is cp_pre_screen.h's for pre_screenjorek_f32 and cp_pre_screenflat.h's for pre_screenjorek_flat_f32:
 *   - PRE_E_NULL for a null pointer (fields, Rb, a kernel, coef, s, its q / score / count, a view's ptr), an empty extent
 *     or count_ld < B;
 *   - PRE_E_RANGE for eq outside [0, 1], nk outside [1, PRE_SCREEN_MAX_LEVELS] or a negative crop;
 *   - PRE_E_UNSUPPORTED before any launch for a layout the form does not take (R's view included), operator weight off
 *     the 7-point star and the flags the form does not take;
 *   - PRE_E_SHAPE as in the two headers;
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`.
 */
#ifndef CP_PRE_SCREENJOREK_H
#define CP_PRE_SCREENJOREK_H

#include <stdint.h>

#include "cp_pre_screen.h"
#include "cp_pre_screenflat.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SCREENJOREK_ABI_VERSION 1
int pre_screenjorek_abi_version(void);  /* == PRE_SCREENJOREK_ABI_VERSION */

/* Ny-fastest fields (every view, Rb and the modulation with unit stride on Y, Y % 4 == 0): r = equation `eq` of
 * pre_residual_jorek_f32, Joint/JOREK_residuals_CP.py:210-243, screened as Joint/JOREK_residuals_CP.py:297-308 does. */
int pre_screenjorek_f32(int eq, const pre_field_t fields[3], const pre_field_t *Rb,
                        const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                        const float coef[4], const pre_screen_t *s,
                        int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* Nt-fastest fields - the layout the script holds: vars[BS,F,Nx,Ny,Nt] dense, each field its permute(0,3,1,2) view (sT == 1,
 * sY == T, Rb likewise): r = equation `eq` of pre_residual_jorek_f32, Joint/JOREK_residuals_CP.py:210-243, screened as
 * Joint/JOREK_residuals_CP.py:297-308 does. */
int pre_screenjorek_flat_f32(int eq, const pre_field_t fields[3], const pre_field_t *Rb,
                             const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                             const float coef[4], const pre_screenflat_t *s,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_SCREENJOREK_H */
