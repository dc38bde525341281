/* cp_pre_pair.h - C ABI of libcp_pre_pair.so: data-driven residual scores in ONE streaming pass.
 *
 * Every Marginal/ and Joint/ script of the reference evaluates its residual twice - on the ground truth and on the
 * surrogate's prediction - and scores the difference (the "Data-Driven" calibration):
 *   cal_pred_residual = residual(cal_pred ...); cal_out_residual = residual(cal_out ...)   Marginal/NS_Residuals_CP.py:284-287
 *   ncf_scores = np.abs(cal_out_residual - cal_pred_residual)                              Marginal/NS_Residuals_CP.py:289
 *   modulation = modulation_func(cal_out_residual, cal_pred_residual)                      Joint/Burgers_Residuals_CP.py:219-220
 * Every score the scripts form (|a - b|, std(a - b), max |a - b| / sigma) depends on d = r(a) - r(b) only.  The entries
 * below read BOTH field sets in one pass of the star march (star_march.h) and write d (or |d| under PRE_FLAG_ABS):
 * 4*(2F + 1) bytes per cell instead of 4*(F + 1) twice plus 12 for the difference pass.
 *
 * Conventions (those of cp_pre_hip.h, whose types, flags and error codes this header uses):
 *   - set `a` is r(y) (the truth), set `b` is r(y_hat) (the prediction); each half of the functor is rounded to fp32
 *     before the subtraction, as numpy subtracts the two residual arrays; |.| is applied after the subtraction;
 *   - the two sets have independent int64 strides (any views sharing one unit-stride axis with `out`, as the twin entry
 *     of cp_pre_hip.h requires); operator kernels and scalars are those of the single-set twin;
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`;
 *   - PRE_E_UNSUPPORTED where the twin returns it (a kernel off the 7-point star, no shared unit-stride axis, an extent
 *     the fused twin does not take), and for NS momentum / MHD continuity whose operators fit neither the reference's
 *     tap structure nor its Ny-fixed form after the axis relabelling (the general-star paired kernel would spill
 *     registers): the caller then runs two single-set passes and a difference;
 *   - PRE_E_NULL for a null pointer or an empty extent, PRE_E_SHAPE for an `out` whose addressed range overlaps the
 *     range of an input view (the pass would read what it has already written).  The check compares BOUNDING byte
 *     ranges (first to last element each view addresses, the halo rows included under PRE_FLAG_HALO_X), not the
 *     elements touched: an `out` interleaved with the inputs - one slot of a stacked buffer that also holds them - is
 *     refused although it shares no element with them, where the single-set twin accepts it.  Write into a separate
 *     buffer, or run the two single-set passes.  A view whose offsets, in elements or in bytes, leave int64 (or whose
 *     range leaves the address space) is PRE_E_SHAPE too: it has no range to compare;
 * Non-finite values reach the cells they reach through the two single-set passes; inf - inf = NaN as in numpy.
 */
#ifndef CP_PRE_PAIR_H
#define CP_PRE_PAIR_H

#include <stdint.h>

#include "cp_pre_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_PAIR_ABI_VERSION 1
int pre_pair_abi_version(void);     /* == PRE_PAIR_ABI_VERSION */

/* pre_stencil3d_f32 on both sets: out = S(a) - S(b), S the tap list (host arrays, 3 offsets per tap).
 * Marginal/Wave_Residuals_CP.py:216-219 (residual(cal_pred...), residual(cal_out...), np.abs of the difference).
 * Star-shaped taps only (else PRE_E_UNSUPPORTED); the <= 3 columns beyond a multiple of 4 of an odd-width contiguous
 * axis are computed by a strided tail kernel, as the twin does (not under PRE_FLAG_HALO_X). */
int pre_pair_stencil3d_f32(const pre_field_t *a, const pre_field_t *b, const pre_out_t *out,
                           const float *tap_w /*host*/, const int32_t *tap_off /*host, 3*ntaps*/, int ntaps,
                           int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* pre_stencil2d_f32 on both sets ([B,T,X], strides {sB,sT,sX}, 2 offsets per tap).
 * Marginal/Advection_Residuals_CP.py:234-235 with the data-driven twin of Marginal/Wave_Residuals_CP.py:216-219. */
int pre_pair_stencil2d_f32(const float *a, const int64_t a_strides[3], const float *b, const int64_t b_strides[3],
                           float *out, const int64_t out_strides[3],
                           const float *tap_w /*host*/, const int32_t *tap_off /*host, 2*ntaps*/, int ntaps,
                           int64_t B, int64_t T, int64_t X, int flags, void *stream);

/* pre_residual_linear2_f32 on both sets: out = (Ka(a0) + ratio*Kb(a1)) - (Ka(b0) + ratio*Kb(b1)).
 * NS continuity, Marginal/NS_Residuals_CP.py:282-283; MHD gauss, Marginal/MHD_Residuals_CP.py:347-348.
 * a, b: {f0, f1}. */
int pre_pair_linear2_f32(const pre_field_t a[2], const pre_field_t b[2], const pre_out_t *out,
                         const float *K_a, const float *K_b, float ratio,
                         int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* pre_residual_ns_momentum_f32 on both sets.  Marginal/NS_Residuals_CP.py:286-289, Joint/NS_Residuals_CP.py:286-290.
 * a, b: {u, v, p}.  PRE_FLAG_INTERIOR_T, PRE_FLAG_OUT_INTERIOR_T and PRE_FLAG_HALO_X as for the twin (halo rows of
 * both sets are read). */
int pre_pair_ns_momentum_f32(const pre_field_t a[3], const pre_field_t b[3], const pre_out_t *out,
                             const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                             float dt, float dx, float dy, float nu,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* pre_residual_mhd_f32(eq = 0, continuity) on both sets.  Marginal/MHD_Residuals_CP.py:327-328; a, b: {rho, u, v}. */
int pre_pair_mhd_continuity_f32(const pre_field_t a[3], const pre_field_t b[3], const pre_out_t *out,
                                const float *K_t, const float *K_x, const float *K_y, double gamma,
                                int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* pre_residual_burgers_f32 on both sets ([B,T,X]).  Joint/Burgers_Residuals_CP.py:217-220. */
int pre_pair_burgers_f32(const float *a, const int64_t a_strides[3], const float *b, const int64_t b_strides[3],
                         float *out, const int64_t out_strides[3],
                         const float *K_t, const float *K_x, const float *K_xx,
                         float dx, float dt, float nu, float c3,
                         int64_t B, int64_t T, int64_t X, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_PAIR_H */
