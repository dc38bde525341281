/* cp_pre_bcres.h - C ABI of libcp_pre_bcres.so: the fused PDE residuals of cp_pre_hip.h under boundary conditions on the
 * x-y rim, in one streaming pass.
 *
 * Every residual of cp_pre_hip.h evaluates its stencils against zero padding, so the callers crop the outer ring in x and
 * y.  The NS, MHD, wave and Burgers data of the reference are periodic in space; Utils/boundary_conditions.py
 * (BoundaryManager.pad_signal) pads the last two axes of a [BS,Nt,Nx,Ny] field by the rule of each side.  Each entry below
 * computes
 *     r_bc(fields) = r_zero_pad( pad(f) for f in fields )[..., :, 1:-1, 1:-1]
 * without the padded copies: the same march and the same functors as pre_residual_*_f32 (compiled with the same flags, so
 * a cell whose star stays inside the grid gets the same bits), with the out-of-domain neighbour of a rim cell read from
 * the mapped in-domain cell or taken as the side's constant.  The time axis keeps its zero padding: planes t = -1 and
 * t = T are zero, their padded ring included.
 *
 * Conventions (types, flags and error codes are those of cp_pre_hip.h):
 *   - `bc` (host): pre_bc_t, mode / value for left, right (columns, Ny) and top, bottom (rows, Nx).  PRE_BC_PERIODIC on a
 *     high side reads index 0: a true wrap.  The same condition and constant applies to every field of a residual;
 *   - the 1-D family ([B,T,X] fields): left / right act on Nx, top / bottom are ignored - the rows (time) take the
 *     constant 0, which is the zero padding;
 *   - every view needs unit stride on its last axis and an extent there that is a multiple of 4; the conditions are tied
 *     to the axes, so nothing is relabelled: anything else is PRE_E_UNSUPPORTED and the caller pads, runs the zero-pad
 *     entry and crops;
 *   - flags: PRE_FLAG_ABS and PRE_FLAG_INTERIOR_T keep their meaning; PRE_FLAG_HALO_X and PRE_FLAG_OUT_INTERIOR_T are
 *     PRE_E_UNSUPPORTED;
 *   - PRE_E_NULL for a null pointer or an empty extent; PRE_E_RANGE for an unknown mode, fewer than 2 cells along an axis
 *     with a PRE_BC_REFLECT side, eq outside [0, 3] or in-plane offsets beyond 32 bits; PRE_E_UNSUPPORTED for an operator
 *     kernel with weight off the 7-point star;
 *   - every functor is built in the reference's tap structure and the y-fixed one, and in the general star except for MHD
 *     momentum and MHD energy (eq 1, 2): their general-star instantiations need scratch memory and are not built, the
 *     entry returns PRE_E_UNSUPPORTED before any launch.  No instantiation that is built uses scratch
 *     (profiles/bcres/resources.txt);
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`; all decisions above are made on the host
 *     before anything is launched.
 */
#ifndef CP_PRE_BCRES_H
#define CP_PRE_BCRES_H

#include <stdint.h>

#include "cp_pre_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_BCRES_ABI_VERSION 1
int pre_bcres_abi_version(void);        /* == PRE_BCRES_ABI_VERSION */

/* out = K(pad(in)): any 3x3x3 star kernel (27 host floats, axes (Nt,Nx,Ny)), taps along Nt included (PRE_Wave) */
int pre_bcres_linear1_f32(const pre_field_t *in, const pre_out_t *out, const float *K, const pre_bc_t *bc,
                          int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
/* out = K_a(pad(f0)) + ratio * K_b(pad(f1)): NS continuity, MHD gauss (pre_residual_linear2_f32) */
int pre_bcres_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const pre_out_t *out,
                          const float *K_a, const float *K_b, float ratio, const pre_bc_t *bc,
                          int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
/* pre_residual_ns_momentum_f32 on the padded fields */
int pre_bcres_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p, const pre_out_t *out,
                              const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                              float dt, float dx, float dy, float nu, const pre_bc_t *bc,
                              int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
/* pre_residual_mhd_f32 on the padded fields; eq: 0 continuity, 1 momentum, 2 energy, 3 induction */
int pre_bcres_mhd_f32(int eq, const pre_field_t fields[6], const pre_out_t *out,
                      const float *K_t, const float *K_x, const float *K_y, double gamma, const pre_bc_t *bc,
                      int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
/* the 1-D family on [B,T,X] (strides {sB,sT,sX}, sX == 1), 3x3 kernels (9 host floats, axes (Nt,Nx)) */
int pre_bcres_burgers_f32(const float *u, const int64_t in_strides[3], float *out, const int64_t out_strides[3],
                          const float *K_t, const float *K_x, const float *K_xx,
                          float dx, float dt, float nu, float c3, const pre_bc_t *bc,
                          int64_t B, int64_t T, int64_t X, int flags, void *stream);
/* out = K(pad(in)): any cross-shaped 3x3 kernel on [B,T,X] (the advection kernel D_t + c D_x) */
int pre_bcres_linear1_rows_f32(const float *in, const int64_t in_strides[3], float *out, const int64_t out_strides[3],
                               const float *K, const pre_bc_t *bc,
                               int64_t B, int64_t T, int64_t X, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_BCRES_H */
