/* cp_pre_vjp.h - C ABI of libcp_pre_vjp.so: the backward pass of physics-informed residual losses.
 *
 * The reference trains its surrogates with the PDE residual in the loss and calls loss.backward() on the device:
 *   PI_loss(pred)  = residual(pred).pow(2).mean()                       Physics_Informed/Wave_FNO_PISL.py:213-214
 *   PISL(pred, yy) = (residual(pred) - residual(yy)).pow(2).mean()      Physics_Informed/Wave_FNO_PISL.py:216-217
 * With an operator D(f)(x) = sum_k w_k f(x+k) (zero padding) the adjoint is D^T(g)(x) = sum_k w_k g(x-k), the same star
 * with mirrored taps.  For the loss, the gradient arriving at the residual is g = s * m * r: r the uncropped residual the
 * forward pass wrote (r(pred) - r(yy) for PISL), m the 0/1 mask of the cells the loss averages over, s = 2 / N * upstream.
 * Each pre_vjp_*_f32 entry below is ONE streaming pass that reads g (and the fields the residual is non-linear in) once
 * and writes the gradient of every field once; pre_vjp_sumsq_f32 is the loss value itself.
 *
 * Conventions (types, error codes of cp_pre_hip.h):
 *   - g is read as stored; the mask (PRE_VJP_CROP: the first and last cell of every residual axis - T, X, Y of a
 *     [B,T,X,Y] view, T and X of a [B,T,X] view - count as 0) and the scale are applied on load, by a select: a
 *     non-finite value outside the crop does not reach the gradient;
 *   - the scale is host_scale * (*dev_scale); dev_scale may be NULL (= 1).  It is a DEVICE pointer: backward() hands
 *     the upstream gradient as a 0-d device tensor, which is thus never read on the host;
 *   - every view needs unit stride on its last axis (contiguous tensors, the vars[:, i] views of a stacked tensor),
 *     else PRE_E_UNSUPPORTED; any width: the last quad of a row that is no multiple of 4 wide is loaded and stored
 *     element by element in the same launch;
 *   - operator kernels are the dense 3x3x3 (3x3) host arrays of the forward entries, used as they are (the reference's
 *     D_y == D_t construction quirk is inherited); a kernel with weight off the 7-point star: PRE_E_UNSUPPORTED;
 *   - PRE_E_NULL for a null pointer or an empty extent; PRE_E_SHAPE for an output whose bounding byte range overlaps
 *     that of an input, or two outputs with one base address (outputs may otherwise interleave: the slots of one
 *     stacked gradient tensor), or a view whose offsets, in elements or in bytes, leave int64;
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`.
 */
#ifndef CP_PRE_VJP_H
#define CP_PRE_VJP_H

#include <stdint.h>

#include "cp_pre_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_VJP_CROP 1             /* mask the rim of every residual axis (boundary=False of the residual methods) */
#define PRE_VJP_VIEW3D 2           /* pre_vjp_sumsq_f32: the view is a [B,T,X] field passed as [1,B,T,X] */
#define PRE_VJP_SUMSQ_WORKSPACE 2048   /* doubles the caller provides to pre_vjp_sumsq_f32 */

#define PRE_VJP_ABI_VERSION 1
int pre_vjp_abi_version(void);     /* == PRE_VJP_ABI_VERSION */

/* out = S^T(scale * m * g), S the tap list (host arrays, 3 offsets per tap) of pre_stencil3d_f32: the gradient of
 * residual(pred) = D(pred), Physics_Informed/Wave_FNO_PISL.py:209-211 (Wave_FNO_PI.py:202-228). */
int pre_vjp_stencil3d_f32(const pre_field_t *g, const pre_out_t *out,
                          const float *tap_w /*host*/, const int32_t *tap_off /*host, 3*ntaps*/, int ntaps,
                          float host_scale, const float *dev_scale /*device, or NULL*/,
                          int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* The same on [B,T,X] (strides {sB,sT,sX}, 2 offsets per tap): the advection loss,
 * Physics_Informed/Advection_FNO_PI.py:207-217. */
int pre_vjp_stencil2d_f32(const float *g, const int64_t g_strides[3], float *out, const int64_t out_strides[3],
                          const float *tap_w /*host*/, const int32_t *tap_off /*host, 2*ntaps*/, int ntaps,
                          float host_scale, const float *dev_scale,
                          int64_t B, int64_t T, int64_t X, int flags, void *stream);

/* r = Ka(a) + ratio*Kb(b) (NS continuity, Marginal/NS_Residuals_CP.py:222-228; MHD gauss):
 * out[0] = Ka^T(scale*m*g), out[1] = ratio * Kb^T(scale*m*g), one read of g. */
int pre_vjp_linear2_f32(const pre_field_t *g, const pre_out_t out[2],
                        const float *K_a, const float *K_b, float ratio,
                        float host_scale, const float *dev_scale,
                        int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* Burgers, r = dx*D_t(u) + dt*u*D_x(u) - nu*c3*D_xx(u) on [B,T,X] (Joint/Burgers_Residuals_CP.py:171-187), gg = scale*m*g:
 *   du = dx*D_t^T(gg) + dt*gg*D_x(u) + dt*D_x^T(gg*u) - nu*c3*D_xx^T(gg). */
int pre_vjp_burgers_f32(const float *g, const int64_t g_strides[3], const float *u, const int64_t u_strides[3],
                        float *du, const int64_t du_strides[3],
                        const float *K_t, const float *K_x, const float *K_xx,
                        float dx, float dt, float nu, float c3,
                        float host_scale, const float *dev_scale,
                        int64_t B, int64_t T, int64_t X, int flags, void *stream);

/* NS momentum (Marginal/NS_Residuals_CP.py:231-240), a = dx*dy, b = dt*dy, c = dt*dx, n = nu*dt, gg = scale*m*g:
 *   out[0] = du = a*D_t^T(gg) - n*L^T(gg) + gg*(b*D_x(u) + c*D_x(v)) + b*D_x^T(gg*u) + c*D_y^T(gg*v)
 *   out[1] = dv = a*D_t^T(gg) - n*L^T(gg) + gg*(c*D_y(u) + b*D_y(v)) + c*D_x^T(gg*u) + b*D_y^T(gg*v)
 *   out[2] = dp = b*D_x^T(gg) + c*D_y^T(gg)
 * in ONE launch: three input streams (g, u, v; p is not read), three output streams.  uv: {u, v}. */
int pre_vjp_ns_momentum_f32(const pre_field_t *g, const pre_field_t uv[2], const pre_out_t out[3],
                            const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                            float dt, float dx, float dy, float nu,
                            float host_scale, const float *dev_scale,
                            int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* *out = sum(m * r^2) in fp64: the numerator of residual(pred).pow(2).mean(), Physics_Informed/Wave_FNO_PISL.py:213-217.
 * Deterministic: per-workgroup fp64 partials in `workspace` (PRE_VJP_SUMSQ_WORKSPACE doubles, device), a second stage
 * that adds them in a fixed order, no floating-point atomics; the same view gives the same bits every time. */
int pre_vjp_sumsq_f32(const pre_field_t *r, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                      double *workspace /*device*/, double *out /*device*/, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_VJP_H */
