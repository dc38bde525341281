/* cp_pre_vjpflatmhd.h - C ABI of libcp_pre_vjpflatmhd.so: the vector-Jacobian products of cp_pre_vjpmhd.h for Nt-FASTEST
 * views of the ideal-MHD residuals - the layout the reference's MHD callers hold: a surrogate's output is
 * [BS,F,Nx,Ny,Nt] and the residuals are evaluated on pred.permute(0,1,4,2,3) (Joint/MHD_Residuals_CP.py,
 * Marginal/MHD_Residuals_CP.py).
 *
 * Each pre_vjpflatmhd_*_f32 entry mirrors its cp_pre_vjpmhd.h counterpart argument for argument; the formulas, the order
 * of the fields, the null and the overlap rules are the ones written there.  B, T, X, Y are the caller's LOGICAL extents,
 * as in cp_pre_vjpflat.h: the library relabels the axes (it marches over X and merges Y and T into one row of Y*T cells)
 * and the operator stars with them.  The march is the merged-row march of libcp_pre_vjpflat.so.
 *
 * Conventions (types, error codes of cp_pre_hip.h; flags of cp_pre_vjp.h):
 *   - g is read as stored; the mask (PRE_VJP_CROP: the first and last cell of T, X and Y count as 0) and the scale
 *     host_scale * (*dev_scale) (dev_scale a DEVICE pointer or NULL) are applied on load, by a select per logical cell;
 *   - padding is zero; g q (q = 1 / rho) is 0 outside the view, never 0 * inf; NaN and inf inside it propagate as they are;
 *   - accepted layout, that of cp_pre_vjpflat.h: g, every field and every output have sT == 1, sY == T and sX == Y*T (any
 *     sB), (Y * T) % 4 == 0 and T < 96; everything else is PRE_E_UNSUPPORTED, as are operator weight off the 7-point star
 *     and any flag but PRE_VJP_CROP;
 *   - PRE_E_NULL for a null pointer or an empty extent; PRE_E_SHAPE for an output whose bounding byte range overlaps that
 *     of ANY input of the entry (whichever launch reads it), two outputs with one base address, or a merged row beyond
 *     2^30 cells;
 *   - every refusal is returned before any launch: momentum and energy are TWO launches each, split by output group as in
 *     cp_pre_vjpmhd.h, and all views of both are checked before the first;
 *   - no atomics: the same views give the same bytes on every run; nothing allocates, nothing synchronises.
 *
 * Tap structures.  The kernels are compiled for the tap structures the forward march has for this layout: the reference's
 * construction (D_t and D_y with taps along Nt only, D_x along Nx only), D_y along Ny (y_axis_fix), and general 7-point
 * stars.  The first two serve all four equations.  With general stars an instantiation that would need scratch memory is
 * not built and its entry returns PRE_E_UNSUPPORTED (pre_vjpflatmhd_supported says so without any views).
 */
#ifndef CP_PRE_VJPFLATMHD_H
#define CP_PRE_VJPFLATMHD_H

#include <stdint.h>

#include "cp_pre_vjpmhd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_VJPFLATMHD_ABI_VERSION 1
int pre_vjpflatmhd_abi_version(void);  /* == PRE_VJPFLATMHD_ABI_VERSION */

/* PRE_OK if the entry of equation `eq` (PRE_VJPMHD_EQ_*) has an instantiation for the tap structure of these kernels,
 * PRE_E_UNSUPPORTED if not (or weight off the star), PRE_E_RANGE for another eq, PRE_E_NULL.  Host only. */
int pre_vjpflatmhd_supported(int eq, const float *K_t, const float *K_x, const float *K_y);

/* fields {rho, u, v}; one launch */
int pre_vjpflatmhd_continuity_f32(const pre_field_t *g, const pre_field_t fields[3], const pre_out_t out[3],
                                  const float *K_t, const float *K_x, const float *K_y,
                                  float host_scale, const float *dev_scale /*device, or NULL*/,
                                  int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* fields {u, v, Bx, By}; one launch */
int pre_vjpflatmhd_induction_f32(const pre_field_t *g, const pre_field_t fields[4], const pre_out_t out[4],
                                 const float *K_t, const float *K_x, const float *K_y,
                                 float host_scale, const float *dev_scale,
                                 int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* fields {rho, u, v, p, Bx, By}; launch A reads g, u, v and writes du, dv; launch B reads g, rho, p, Bx, By and writes
 * d rho, dp, dBx, dBy */
int pre_vjpflatmhd_momentum_f32(const pre_field_t *g, const pre_field_t fields[6], const pre_out_t out[6],
                                const float *K_t, const float *K_x, const float *K_y,
                                float host_scale, const float *dev_scale,
                                int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* fields {rho, u, v, p, Bx, By} (rho is checked like the others but not read); launch A reads g, p, Bx, By and writes
 * d rho, du, dv; launch B reads g, u, v, Bx, By and writes dp, dBx, dBy */
int pre_vjpflatmhd_energy_f32(const pre_field_t *g, const pre_field_t fields[6], const pre_out_t out[6],
                              const float *K_t, const float *K_x, const float *K_y, double gamma,
                              float host_scale, const float *dev_scale,
                              int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_VJPFLATMHD_H */
