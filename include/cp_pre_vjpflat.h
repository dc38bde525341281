/* cp_pre_vjpflat.h - C ABI of libcp_pre_vjpflat.so: the vector-Jacobian products of cp_pre_vjp.h for Nt-FASTEST views of
 * the 2-D residuals - the layout the reference's training scripts backpropagate through:
 *   field[:, 0, 1:-1, 1:-1, 1:-1].permute(0, 3, 1, 2) -> residual(...).pow(2).mean()   Physics_Informed/Wave_FNO_PISL.py:209-217
 *   residual_momentum(pred.permute(0,1,4,2,3))                                         Joint/NS_Residuals_CP.py:282-305
 * Each pre_vjpflat_*_f32 entry is ONE streaming pass over a [B,T,X,Y] batch whose memory is [B,X,Y,T]: it reads the gradient
 * g arriving at the residual (and the fields the residual is non-linear in) once and writes the gradient of every field
 * once, in the same memory order.  Shapes and taps are the caller's LOGICAL [B,T,X,Y]; the library relabels the axes (it
 * marches over X and merges Y and T into one row of Y*T cells).  The entries mirror those of cp_pre_vjp.h argument for
 * argument; the formulas are the ones written there.
 *
 * Conventions (types, error codes of cp_pre_hip.h; flags of cp_pre_vjp.h):
 *   - g is read as stored; the mask (PRE_VJP_CROP: the first and last cell of T, X and Y count as 0) and the scale are
 *     applied on load, by a select per logical cell: a non-finite value outside the crop does not reach the gradient;
 *   - the scale is host_scale * (*dev_scale); dev_scale may be NULL (= 1).  It is a DEVICE pointer and is never read on
 *     the host;
 *   - padding is zero (the adjoint of a zero-padded correlation); a gradient is written for every cell of the view, the
 *     rim included;
 *   - accepted layout: g, every output and the u, v views of NS momentum have sT == 1, sY == T and sX == Y*T (any sB),
 *     (Y * T) % 4 == 0 and T < 96; everything else - a unit-stride last axis included: that is libcp_pre_vjp.so's - is
 *     PRE_E_UNSUPPORTED before any launch, as are operator weight off the 7-point star and any flag but PRE_VJP_CROP;
 *   - PRE_E_NULL for a null pointer or an empty extent; PRE_E_SHAPE for an output whose bounding byte range overlaps that
 *     of an input, two outputs with one base address, a view whose offsets, in elements or in bytes, leave int64, a
 *     merged row beyond 2^30 cells or a tap offset beyond +-3;
 *   - no atomics: the same view gives the same bytes on every run; nothing allocates, nothing synchronises, all work is
 *     enqueued on `stream`.
 */
#ifndef CP_PRE_VJPFLAT_H
#define CP_PRE_VJPFLAT_H

#include <stdint.h>

#include "cp_pre_vjp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_VJPFLAT_ABI_VERSION 1
int pre_vjpflat_abi_version(void);  /* == PRE_VJPFLAT_ABI_VERSION */

/* out = S^T(scale * m * g), S the tap list (host arrays, 3 offsets per tap on the logical (T,X,Y)) of pre_stencil3d_f32:
 * the gradient of PI_loss / PISL on the script's Nt-fastest view, Physics_Informed/Wave_FNO_PISL.py:209-217. */
int pre_vjpflat_stencil3d_f32(const pre_field_t *g, const pre_out_t *out,
                              const float *tap_w /*host*/, const int32_t *tap_off /*host, 3*ntaps*/, int ntaps,
                              float host_scale, const float *dev_scale /*device, or NULL*/,
                              int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* r = Ka(a) + ratio*Kb(b) (NS continuity on pred.permute(0,1,4,2,3), Joint/NS_Residuals_CP.py:222-228):
 * out[0] = Ka^T(scale*m*g), out[1] = ratio * Kb^T(scale*m*g), one read of g. */
int pre_vjpflat_linear2_f32(const pre_field_t *g, const pre_out_t out[2],
                            const float *K_a, const float *K_b, float ratio,
                            float host_scale, const float *dev_scale,
                            int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* NS momentum on pred.permute(0,1,4,2,3) (Joint/NS_Residuals_CP.py:231-240): out = {du, dv, dp} of
 * pre_vjp_ns_momentum_f32, in ONE launch: three input streams (g, u, v; p is not read), three output streams.  uv: {u, v}. */
int pre_vjpflat_ns_momentum_f32(const pre_field_t *g, const pre_field_t uv[2], const pre_out_t out[3],
                                const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                float dt, float dx, float dy, float nu,
                                float host_scale, const float *dev_scale,
                                int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_VJPFLAT_H */
