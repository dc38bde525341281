/* cp_pre_screenpair.h - C ABI of libcp_pre_screenpair.so: the calibrated-set screens of cp_pre_screen.h (Ny-fastest fields)
 * and cp_pre_screenflat.h (Nt-fastest fields) for the data-driven scores of cp_pre_pair.h - the question every Joint/
 * script of the reference asks of its held-out pairs after calibrating on r(y) - r(y_hat):
 *   Joint/NS_Residuals_CP.py:289-290, 307-313, the same lines of Joint/MHD_Residuals_CP.py,
 *   Joint/Burgers_Residuals_CP.py:217-220; Other_UQ/Evaluation/Eval.py:278-281 for the solution-space analogue.
 * Each entry is ONE streaming pass over BOTH field sets of a [B,T,X,Y] batch that evaluates the two residuals in registers
 * and reduces their difference, per sample, to
 *   d             = fl(fl(r(a)) - fl(r(b)))     each half rounded to fp32 before the subtraction, as libcp_pre_pair.so does
 *   score[b]      = max over the counted cells of |d| / m
 *   count[k][b]   = number of counted cells with |d| <= fl(q[k] * m)   (k < nk <= PRE_SCREEN_MAX_LEVELS)
 * Neither residual nor d is written.
 *
 * Semantics: this is the one-sided test on the difference - what pre_pair_*_f32, the joint score and pre_cov_levels_f32
 * give in three passes.  It is NOT the reference's two-sided form c - hw <= y <= c + hw on the two residual arrays: the two
 * can differ in a cell that sits within rounding of the band's edge.
 *
 * Conventions:
 *   - set `a` is the truth (r(y)), set `b` the prediction (r(y_hat)); the two sets have independent strides and may be
 *     the same memory (then every score is +0 and every cell with q[k] * m >= 0 is inside);
 *   - each entry takes the arguments of its single-set twin (pre_screen_*_f32, pre_screenflat_*_f32) with the twin's field
 *     views replaced by the two sets, `a` first: one view each for stencil3d, arrays of 2 (f0, f1) for linear2, of 3
 *     (u, v, p) for NS momentum and of 3 (rho, u, v: channels 0, 1, 2) for MHD continuity.  pre_screen_t and
 *     pre_screenflat_t are unchanged;
 *   - everything else - accumulation, the crop by select, the guarded divide, sticky NaN, the non-finite contract,
 *     hw = q[k] * m, `q` on the device, the accepted layouts - is cp_pre_screen.h's for the pre_screenpair_*_f32 entries and
 *     cp_pre_screenflat.h's for the pre_screenpair_flat_*_f32 entries, and holds for every view of both sets.
 *     PRE_FLAG_HALO_X and PRE_FLAG_INTERIOR_T apply to both sets on the Ny-fastest march: rows -1 and X of every view of
 *     both sets are read; the flat entries take PRE_FLAG_INTERIOR_T only;
 *   - PRE_E_UNSUPPORTED before any launch wherever the twin returns it, and for NS momentum / MHD continuity whose
 *     operators fit neither the reference's tap structure nor its y-fixed form (the general-star paired kernels are not
 *     built, as in libcp_pre_pair.so), and for the y-fixed form of NS momentum on Nt-fastest fields (it would not fit the
 *     registers): the caller takes its three-pass route;
 *   - PRE_E_NULL, PRE_E_RANGE, PRE_E_SHAPE as in the two headers;
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`.
 */
#ifndef CP_PRE_SCREENPAIR_H
#define CP_PRE_SCREENPAIR_H

#include <stdint.h>

#include "cp_pre_screen.h"
#include "cp_pre_screenflat.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SCREENPAIR_ABI_VERSION 1
int pre_screenpair_abi_version(void);  /* == PRE_SCREENPAIR_ABI_VERSION */

/* ---- Ny-fastest fields (every view and the modulation with unit stride on Y, Y % 4 == 0) ---- */

/* d = S(a) - S(b), S a tap list as pre_screen_stencil3d_f32 takes it (star-shaped): the wave residual on truth and
 * prediction, Other_UQ/Evaluation/Eval.py:278-281. */
int pre_screenpair_stencil3d_f32(const pre_field_t *a, const pre_field_t *b,
                                 const float *tap_w /*host*/, const int32_t *tap_off /*host, 3*ntaps*/, int ntaps,
                                 const pre_screen_t *s,
                                 int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* d = (Ka(a0) + ratio*Kb(a1)) - (Ka(b0) + ratio*Kb(b1)): NS continuity, MHD gauss on both sets,
 * Joint/NS_Residuals_CP.py:289-290, 307-313. */
int pre_screenpair_linear2_f32(const pre_field_t a[2], const pre_field_t b[2], const float *K_a, const float *K_b, float ratio,
                               const pre_screen_t *s,
                               int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* d = the NS momentum residual of pre_residual_ns_momentum_f32 on a = {u, v, p} less that on b,
 * Joint/NS_Residuals_CP.py:289-290, 307-313. */
int pre_screenpair_ns_momentum_f32(const pre_field_t a[3], const pre_field_t b[3],
                                   const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                   float dt, float dx, float dy, float nu, const pre_screen_t *s,
                                   int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* d = the MHD continuity residual (pre_residual_mhd_f32, eq 0) on a = {rho, u, v} less that on b,
 * Joint/MHD_Residuals_CP.py:289-290, 307-313. */
int pre_screenpair_mhd_continuity_f32(const pre_field_t a[3], const pre_field_t b[3],
                                      const float *K_t, const float *K_x, const float *K_y, double gamma,
                                      const pre_screen_t *s,
                                      int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* ---- Nt-fastest fields (every view with sT == 1 and sY == T, the modulation likewise; cp_pre_screenflat.h) ---- */

/* pre_screenpair_stencil3d_f32 on the merged-row march, Other_UQ/Evaluation/Eval.py:278-281. */
int pre_screenpair_flat_stencil3d_f32(const pre_field_t *a, const pre_field_t *b,
                                      const float *tap_w /*host*/, const int32_t *tap_off /*host, 3*ntaps*/, int ntaps,
                                      const pre_screenflat_t *s,
                                      int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* pre_screenpair_linear2_f32 on the merged-row march, Joint/NS_Residuals_CP.py:289-290, 307-313. */
int pre_screenpair_flat_linear2_f32(const pre_field_t a[2], const pre_field_t b[2], const float *K_a, const float *K_b,
                                    float ratio, const pre_screenflat_t *s,
                                    int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* pre_screenpair_ns_momentum_f32 on the merged-row march: the layout Joint/NS_Residuals_CP.py:289-290, 307-313 holds. */
int pre_screenpair_flat_ns_momentum_f32(const pre_field_t a[3], const pre_field_t b[3],
                                        const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                        float dt, float dx, float dy, float nu, const pre_screenflat_t *s,
                                        int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* pre_screenpair_mhd_continuity_f32 on the merged-row march: the layout Joint/MHD_Residuals_CP.py:289-290, 307-313 holds. */
int pre_screenpair_flat_mhd_continuity_f32(const pre_field_t a[3], const pre_field_t b[3],
                                           const float *K_t, const float *K_x, const float *K_y, double gamma,
                                           const pre_screenflat_t *s,
                                           int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_SCREENPAIR_H */
