/* cp_pre_screencellspair.h - C ABI of libcp_pre_screencellspair.so: the per-cell screens of cp_pre_screencells.h for the
 * data-driven scores of cp_pre_screenpair.h - how every Marginal/ script of the reference validates its held-out pairs: a
 * quantile per cell at ten alphas calibrated on |r(y) - r(y_hat)|, and then, per alpha, is r(y) of every held-out pair
 * inside r(y_hat) +- qhat[k][cell]:
 *   Marginal/NS_Residuals_CP.py:282-312, Marginal/MHD_Residuals_CP.py:350-392, Marginal/Wave_Residuals_CP.py:219-254
 * Each entry is ONE streaming pass over BOTH field sets of a [B,T,X,Y] batch that evaluates the two residuals in registers
 * and reduces their difference, per sample, to
 *   d             = fl(fl(r(a)) - fl(r(b)))     each half rounded to fp32 before the subtraction (cp_pre_screenpair.h)
 *   score[b]      = max over the counted cells of |d| / m                      (m == 1 without a modulation)
 *   count[k][b]   = number of counted cells with |d| <= hw,  hw = levels[k][cell]        without a modulation,
 *                                                            hw = fl(levels[k][cell] * m[cell])   with one
 * Neither residual nor d is written.  count is what pre_cov_levels_f32 counts on the stored difference with q_ld != 0, per
 * sample.
 *
 * Semantics: the one-sided test on the difference, NOT the reference's two-sided form c - hw <= y <= c + hw on the two
 * residual arrays; the two can differ in a cell that sits within rounding of the band's edge (cp_pre_screenpair.h).
 *
 * Conventions: this header defines no struct of its own.
 *   - the field sets are cp_pre_screenpair.h's: `a` the truth, `b` the prediction, independent strides, one view each for
 *     stencil3d, arrays of 2 (f0, f1) for linear2, of 3 (u, v, p) for NS momentum and of 3 (rho, u, v) for MHD continuity;
 *     the two may be the same memory (then every score is +0 and every cell with levels[k] * m >= 0 is inside);
 *   - the sets are cp_pre_screencells.h's: pre_screencells_t for the Ny-fastest entries, pre_screencellsflat_t for the flat
 *     ones, with that header's layouts, rim and non-finite contract;
 *   - each entry takes the arguments of its twin pre_screenpair_*_f32 with the set descriptor swapped, and everything else -
 *     accumulation, the crop, the flags (PRE_FLAG_HALO_X and PRE_FLAG_INTERIOR_T on the Ny-fastest march, of both sets;
 *     PRE_FLAG_INTERIOR_T alone on the flat one), the checks and their order, for every view of both sets - is the twin's;
 *   - block order: the samples in groups of pre_screencellspair_sample_group(), the sample of a group the fastest block
 *     index (cp_pre_screencells.h).  Speed only;
 *   - PRE_E_UNSUPPORTED before any launch wherever the twin returns it, and for the y-fixed tap structure of NS momentum in
 *     BOTH layouts (with level quads it does not fit the registers): the caller takes its three-pass route;
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`.
 */
#ifndef CP_PRE_SCREENCELLSPAIR_H
#define CP_PRE_SCREENCELLSPAIR_H

#include <stdint.h>

#include "cp_pre_screencells.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SCREENCELLSPAIR_ABI_VERSION 1
int pre_screencellspair_abi_version(void);   /* == PRE_SCREENCELLSPAIR_ABI_VERSION */
int pre_screencellspair_sample_group(void);  /* samples per group of the block order (>= 1), a constant of the build */

/* ---- Ny-fastest fields (every view, the modulation and the level fields with unit stride on Y, Y % 4 == 0) ---- */

/* d = S(a) - S(b), S a tap list (star-shaped): the wave residual, Marginal/Wave_Residuals_CP.py:219-254. */
int pre_screencellspair_stencil3d_f32(const pre_field_t *a, const pre_field_t *b,
                                      const float *tap_w /*host*/, const int32_t *tap_off /*host, 3*ntaps*/, int ntaps,
                                      const pre_screencells_t *s,
                                      int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* d = (Ka(a0) + ratio*Kb(a1)) - (Ka(b0) + ratio*Kb(b1)): NS continuity, MHD gauss, Marginal/NS_Residuals_CP.py:282-312. */
int pre_screencellspair_linear2_f32(const pre_field_t a[2], const pre_field_t b[2], const float *K_a, const float *K_b,
                                    float ratio, const pre_screencells_t *s,
                                    int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* d = the NS momentum residual on a = {u, v, p} less that on b, Marginal/NS_Residuals_CP.py:282-312. */
int pre_screencellspair_ns_momentum_f32(const pre_field_t a[3], const pre_field_t b[3],
                                        const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                        float dt, float dx, float dy, float nu, const pre_screencells_t *s,
                                        int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* d = the MHD continuity residual on a = {rho, u, v} less that on b, Marginal/MHD_Residuals_CP.py:350-392. */
int pre_screencellspair_mhd_continuity_f32(const pre_field_t a[3], const pre_field_t b[3],
                                           const float *K_t, const float *K_x, const float *K_y, double gamma,
                                           const pre_screencells_t *s,
                                           int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* ---- Nt-fastest fields (pred.permute(0,1,4,2,3), the layout the scripts hold: cp_pre_screenflat.h) ---- */

int pre_screencellspair_flat_stencil3d_f32(const pre_field_t *a, const pre_field_t *b,
                                           const float *tap_w /*host*/, const int32_t *tap_off /*host, 3*ntaps*/, int ntaps,
                                           const pre_screencellsflat_t *s,
                                           int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

int pre_screencellspair_flat_linear2_f32(const pre_field_t a[2], const pre_field_t b[2], const float *K_a, const float *K_b,
                                         float ratio, const pre_screencellsflat_t *s,
                                         int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

int pre_screencellspair_flat_ns_momentum_f32(const pre_field_t a[3], const pre_field_t b[3],
                                             const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                             float dt, float dx, float dy, float nu, const pre_screencellsflat_t *s,
                                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

int pre_screencellspair_flat_mhd_continuity_f32(const pre_field_t a[3], const pre_field_t b[3],
                                                const float *K_t, const float *K_x, const float *K_y, double gamma,
                                                const pre_screencellsflat_t *s,
                                                int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_SCREENCELLSPAIR_H */
