/* cp_pre_vjpmhd.h - C ABI of libcp_pre_vjpmhd.so: the backward pass of physics-informed losses on the ideal-MHD residuals
 * (Marginal/MHD_Residuals_CP.py:225-268), the counterpart of cp_pre_vjp.h's NS entries for pre_residual_mhd_f32.
 *
 * Conventions: those of cp_pre_vjp.h.  g is the gradient arriving at the uncropped residual; gg = scale * m * g is formed
 * on load by a select (PRE_VJP_CROP: the first and last cell of T, X and Y count as 0; scale = host_scale * (*dev_scale),
 * dev_scale a DEVICE pointer or NULL).  Every view needs unit stride on its last axis (PRE_E_UNSUPPORTED otherwise), any
 * width.  PRE_E_NULL for a null pointer or an empty extent; PRE_E_SHAPE for an output whose bounding byte range overlaps
 * that of ANY input of the entry (whichever launch reads it), or two outputs with one base address.  Operator kernels
 * are the dense 3x3x3 host arrays of pre_residual_mhd_f32, used as they are; weight off the 7-point star:
 * PRE_E_UNSUPPORTED.  Every refusal is returned before any launch.  Nothing allocates, nothing synchronises, no atomics:
 * the same views give the same bytes every time.
 *
 * Fields are passed in the order of pre_residual_mhd_f32 - (rho, u, v, p, Bx, By), or the subset an equation reads - and
 * out[i] receives the gradient with respect to fields[i].  D^T is the star with mirrored taps, M = D_x - D_y,
 * P = D_x + D_y (folded on the host in double, rounded once), q = 1 / rho.  Outside a view every field reads as the zero
 * padding of the operators; g q there is 0.
 *
 * Tap structures.  The kernels are compiled for the tap structures of the forward march: 0 - the reference's construction
 * (D_t and D_y with taps along Nt only, D_x along Nx only), 1 - D_y along Ny (y_axis_fix), 2 - general 7-point stars.  An
 * instantiation that would need scratch memory is not built: with general stars only momentum is; continuity, induction
 * and energy return PRE_E_UNSUPPORTED (pre_vjpmhd_supported says so without any views).  Momentum and energy are TWO
 * launches each, split by output group (in one launch they need scratch in every structure); all views of both launches
 * are checked before the first.
 */
#ifndef CP_PRE_VJPMHD_H
#define CP_PRE_VJPMHD_H

#include <stdint.h>

#include "cp_pre_vjp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_VJPMHD_ABI_VERSION 1
int pre_vjpmhd_abi_version(void);  /* == PRE_VJPMHD_ABI_VERSION */

/* the equations, numbered as `eq` of pre_residual_mhd_f32 */
#define PRE_VJPMHD_EQ_CONTINUITY 0
#define PRE_VJPMHD_EQ_MOMENTUM 1
#define PRE_VJPMHD_EQ_ENERGY 2
#define PRE_VJPMHD_EQ_INDUCTION 3

/* PRE_OK if the entry of equation `eq` has an instantiation for the tap structure of these kernels, PRE_E_UNSUPPORTED if
 * not (or weight off the star), PRE_E_RANGE for another eq, PRE_E_NULL.  Host only. */
int pre_vjpmhd_supported(int eq, const float *K_t, const float *K_x, const float *K_y);

/* continuity, r = Dt(rho) + u Dx(rho) + rho Dx(u) + v Dy(rho) + rho Dy(v); fields {rho, u, v}; one launch:
 *   d rho = Dt^T gg + Dx^T(gg u) + Dy^T(gg v) + gg (Dx u + Dy v)
 *   du = gg Dx rho + Dx^T(gg rho)         dv = gg Dy rho + Dy^T(gg rho) */
int pre_vjpmhd_continuity_f32(const pre_field_t *g, const pre_field_t fields[3], const pre_out_t out[3],
                              const float *K_t, const float *K_x, const float *K_y,
                              float host_scale, const float *dev_scale /*device, or NULL*/,
                              int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* induction; fields {u, v, Bx, By}; one launch:
 *   du  =  M^T(gg By) + gg P(By)          dv  = -M^T(gg Bx) - gg P(Bx)
 *   dBx = Dt^T gg - gg M(v) - P^T(gg v)   dBy = Dt^T gg + gg M(u) + P^T(gg u) */
int pre_vjpmhd_induction_f32(const pre_field_t *g, const pre_field_t fields[4], const pre_out_t out[4],
                             const float *K_t, const float *K_x, const float *K_y,
                             float host_scale, const float *dev_scale,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* momentum; fields {rho, u, v, p, Bx, By}; sx = 2 Dx Bx + P By, sy = 2 Dy By + P Bx, S = Bx sx + By sy,
 * T = Dt^T gg + Dx^T(gg u) + Dy^T(gg v).
 *   launch A (reads g, u, v):           du = T + gg Dx(u+v)            dv = T + gg Dy(u+v)
 *   launch B (reads g, rho, p, Bx, By): d rho = -gg q^2 (P p - S)      dp = P^T(gg q)
 *                                       dBx = -( gg q sx + 2 Dx^T(gg q Bx) + P^T(gg q By) )
 *                                       dBy = -( gg q sy + 2 Dy^T(gg q By) + P^T(gg q Bx) ) */
int pre_vjpmhd_momentum_f32(const pre_field_t *g, const pre_field_t fields[6], const pre_out_t out[6],
                            const float *K_t, const float *K_x, const float *K_y,
                            float host_scale, const float *dev_scale,
                            int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* energy; fields {rho, u, v, p, Bx, By} (rho is checked like the others but not read: d rho = Dt^T gg);
 * pg = p - (Bx^2 + By^2)/2, A = gamma pg + By^2, C = gamma pg + Bx^2, E = Bx By, W = u Bx + v By, dv = Dx Bx + Dy By,
 * sh = Dy u + Dx v, k = gamma - 2 (formed in double, rounded once).
 *   launch A (reads g, p, Bx, By):      d rho = Dt^T gg
 *                                       du = gg (Dx p + k Bx dv) + Dx^T(gg A) - Dy^T(gg E)
 *                                       dv = gg (Dy p + k By dv) + Dy^T(gg C) - Dx^T(gg E)
 *   launch B (reads g, u, v, Bx, By):   dp  = Dx^T(gg u) + Dy^T(gg v) + gamma gg (Dx u + Dy v)
 *                                       dBx = k (gg u dv + Dx^T(gg W)) + gg ( Bx((2-gamma) Dy v - gamma Dx u) - By sh )
 *                                       dBy = k (gg v dv + Dy^T(gg W)) + gg ( By((2-gamma) Dx u - gamma Dy v) - Bx sh ) */
int pre_vjpmhd_energy_f32(const pre_field_t *g, const pre_field_t fields[6], const pre_out_t out[6],
                          const float *K_t, const float *K_x, const float *K_y, double gamma,
                          float host_scale, const float *dev_scale,
                          int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_VJPMHD_H */
