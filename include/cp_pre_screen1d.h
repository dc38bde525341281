/* cp_pre_screen1d.h - C ABI of libcp_pre_screen1d.so: the calibrated-set screen of cp_pre_screen.h for the 1-D residuals
 * on [B,Nt,Nx] fields, where a sample is one [Nt,Nx] plane.
 *
 * The accept / reject loops that follow a joint calibration of a 1-D surrogate ask of every prediction whether its
 * residual lies inside the set:
 *   the reject-and-resimulate loops      Active_Learning/Burgers_AL_Joint.py:305-379
 *                                        Active_Learning/Advection_AL_Joint.py:291-336
 *                                        Active_Learning/Advection_AL_Marginal.py:169-198,290-311
 * Each pre_screen1d_*_f32 entry is ONE streaming pass over a [B,T,X] batch (T = Nt, X = Nx) that evaluates the residual r
 * in registers (the functors of pre_stencil2d_f32's star form and of pre_residual_burgers_f32, unchanged) and reduces it,
 * per sample, to
 *   score[b]      = max over the counted cells of |r| / m          (ncf_metric_joint, Joint/NS_Residuals_CP.py:318-320)
 *   count[k][b]   = number of counted cells with |r| <= q[k] * m   (k < nk <= PRE_SCREEN_MAX_LEVELS)
 * The residual is never written.  Cells outside the sample are zero padding, as in the residual passes.
 *
 * Both entries take the pre_screen_t of cp_pre_screen.h, read on the two axes of a sample:
 *   - `ct` holds the Nt crop, `cx` the Nx crop: the counted cells are t in [ct, T - ct), x in [cx, X - cx).  `cy` must
 *     be 0 (PRE_E_RANGE otherwise);
 *   - `modulation` m[T,X] is shared by all samples; `mT` holds its Nt stride, `mX` its Nx stride (elements).  NULL means
 *     m == 1.  Its values outside the counted region are never used;
 *   - `strides` are the element strides of `u` on (B, Nt, Nx).  The field needs a unit-stride axis, Nx (strides[2] == 1,
 *     the reference layout) or Nt (strides[1] == 1: `u.permute(0,1,3,2)[:,0]` of the surrogate's native layout), and the
 *     modulation must have unit stride on the same axis.  The star weights are relabelled to the layout, as
 *     pre_residual_burgers_f32 does.
 *
 * Conventions are those of cp_pre_screen.h:
 *   - results are ACCUMULATED: score by an unsigned integer maximum of the fp32 bit pattern (NaN lies above +inf), count
 *     by integer adds.  The caller zeroes both buffers before the first call; repeated calls and overlapping row slabs
 *     (with crops that count every cell once) then compose to the bits of the whole sample, in any order.  `score` is
 *     uint32 [B], `count` uint32 [nk][count_ld], count_ld >= B.  Integer atomics only: the same input gives the same bytes
 *     on every run;
 *   - the non-finite contract: a cell outside the counted region contributes nothing, whatever it holds (masked by a
 *     select).  Inside it, NaN r or m (and 0/0) make the score NaN and the cell outside at every level; m == 0 with
 *     r != 0 gives an inf score and the cell outside;
 *   - hw = q[k] * m is one fp32 multiplication (no fma), the inside test |r| <= hw: what libcp_pre_cov.so computes;
 *   - `q`: DEVICE pointer to nk fp32 levels;
 *   - PRE_E_UNSUPPORTED before any launch for: a tap or an operator weight off the 5-point star of the (Nt, Nx) plane, a
 *     contiguous-axis length that is no multiple of 4, a field or modulation view with no unit-stride axis or whose
 *     unit-stride axes differ, any flag (the caller takes its three-pass route);
 *   - PRE_E_NULL for a null pointer, an empty extent or count_ld < B, PRE_E_RANGE for nk outside
 *     [1, PRE_SCREEN_MAX_LEVELS], a negative crop or cy != 0, PRE_E_SHAPE for T*X >= 2^32 (the counts are 32-bit), a
 *     contiguous axis beyond 2^28 cells or a tap offset beyond +-3;
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`.
 */
#ifndef CP_PRE_SCREEN1D_H
#define CP_PRE_SCREEN1D_H

#include <stdint.h>

#include "cp_pre_screen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SCREEN1D_ABI_VERSION 1
int pre_screen1d_abi_version(void);  /* == PRE_SCREEN1D_ABI_VERSION */

/* r = S(u), S a tap list (host arrays, 2 offsets per tap: Nt, Nx) as pre_stencil2d_f32 takes it: any ConvOperator of
 * Utils/ConvOps_1d.py:150 and the advection residual D_t + (v disc dt/dx) D_x, Marginal/Advection_Residuals_CP.py:156-164,
 * screened as Active_Learning/Advection_AL_Joint.py:291-336 and Active_Learning/Advection_AL_Marginal.py:169-198 do. */
int pre_screen1d_stencil2d_f32(const float *u, const int64_t strides[3], const float *tap_w /*host*/,
                               const int32_t *tap_off /*host, 2*ntaps*/, int ntaps, const pre_screen_t *s,
                               int64_t B, int64_t T, int64_t X, int flags, void *stream);

/* r = dx*D_t(u) + dt*u*D_x(u) - nu*D_xx(u)*c3, the Burgers residual of pre_residual_burgers_f32
 * (Joint/Burgers_Residuals_CP.py:182-187; K_t, K_x, K_xx dense 3x3 host kernels on (Nt, Nx)), screened as
 * Active_Learning/Burgers_AL_Joint.py:305-379 does. */
int pre_screen1d_burgers_f32(const float *u, const int64_t strides[3], const float *K_t, const float *K_x, const float *K_xx,
                             float dx, float dt, float nu, float c3, const pre_screen_t *s,
                             int64_t B, int64_t T, int64_t X, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_SCREEN1D_H */
