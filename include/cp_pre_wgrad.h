/* cp_pre_wgrad.h - C ABI of libcp_pre_wgrad.so: the gradient of a physics-informed residual loss with respect to a
 * TRAINABLE operator kernel, in one streaming pass.
 *
 * The reference's wave scripts train the operator kernel itself (Physics_Informed/Wave_FNO_PI.py:202-210,
 * Wave_FNO_PISL.py:203-211):
 *   D.kernel = D_tt.kernel - (c*dt/dx)**2 * D_xx_yy.kernel;  D.kernel.requires_grad = True
 *   loss = D(field).pow(2).mean();  loss.backward()
 * With r = D(x) (r = D(x) - D(y) = D(x - y) for PISL), D(f)(c) = sum_k K[k] f(c + k - 1) (zero padding), the gradient is
 *   dL/dK[k] = scale * sum_c m_c * g_c * (x - y)(c + k - 1),       g = r,  scale = 2 / N * upstream,
 * 27 (9, 3) masked shifted inner products of two (three) streams.  pre_wgrad_stencil3d_f32 forms them all in ONE pass:
 * g, x and y are each read once (x and y with the halo of a tile), nothing else is read or written but the partial sums.
 *
 * Conventions are those of cp_pre_vjp.h (types, error codes of cp_pre_hip.h):
 *   - g is read as stored; the mask (PRE_VJP_CROP: the first and last cell of every residual axis count as 0; with
 *     PRE_VJP_VIEW3D, a [B,T,X] field passed as [1,B,T,X] with kernel (1,kt,kx), of T and X only) is a select on g:
 *     a non-finite g in the rim does not reach dk.  The rim cells of x and y ARE read (an interior g meets them);
 *   - scale = host_scale * (*dev_scale), formed in fp64; dev_scale is a DEVICE pointer or NULL (= 1): backward() hands
 *     the upstream gradient as a 0-d device tensor, which is never read on the host;
 *   - g, x and y (y may be NULL: the PI loss) share one of two layouts: unit stride on Y with any sB, sT, sX (contiguous
 *     tensors, vars[:, i] views, pitched rows, any width), or the Nt-fastest view, unit stride on T with any sB, sX, sY
 *     (permute(0,3,1,2) of a dense [B,X,Y,T] array, sY == T, sX == Y*T, and the cropped sub-views of one: the view the
 *     reference's scripts pass).  Anything else: PRE_E_UNSUPPORTED before any launch;
 *   - kernel extents kt, kx, ky in {1, 3}; dk is the dense [kt][kx][ky] device array in the LOGICAL order whatever the
 *     layout; other extents, other flags: PRE_E_UNSUPPORTED;
 *   - PRE_E_NULL for a null pointer or an empty extent; PRE_E_SHAPE for an extent beyond int32 or a dk / workspace whose
 *     byte range overlaps that of an input (or each other), or an input view whose offsets, in elements or in bytes,
 *     leave int64;
 *   - deterministic: the grid is a function of the shape alone, every workgroup writes one fp64 partial per tap to
 *     `workspace`, a second stage adds them in a fixed order, applies the scale in fp64 and rounds ONCE to fp32.  No
 *     floating-point atomics, no atomics on dk: the same views give the same bytes every time, on any stream;
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`.
 */
#ifndef CP_PRE_WGRAD_H
#define CP_PRE_WGRAD_H

#include <stdint.h>

#include "cp_pre_hip.h"
#include "cp_pre_vjp.h"            /* PRE_VJP_CROP, PRE_VJP_VIEW3D */

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_WGRAD_WORKSPACE 55296  /* doubles the caller provides: 27 taps x at most 2048 workgroups */

#define PRE_WGRAD_ABI_VERSION 1
int pre_wgrad_abi_version(void);   /* == PRE_WGRAD_ABI_VERSION */

/* dk[it][ix][iy] = scale * sum_c m_c * g_c * (x - y)_{c + (it-kt/2, ix-kx/2, iy-ky/2)},  zero padding,
 * extents kt,kx,ky in {1,3};  y may be NULL (PI loss);  scale = host_scale * (*dev_scale), dev_scale device or NULL */
int pre_wgrad_stencil3d_f32(const pre_field_t *g, const pre_field_t *x, const pre_field_t *y,
                            int kt, int kx, int ky, float host_scale, const float *dev_scale,
                            int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                            double *workspace /*device, PRE_WGRAD_WORKSPACE doubles*/,
                            float *dk /*device, kt*kx*ky*/, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_WGRAD_H */
