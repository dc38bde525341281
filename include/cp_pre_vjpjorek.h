/* cp_pre_vjpjorek.h - C ABI of libcp_pre_vjpjorek.so: the vector-Jacobian products of the reduced-MHD (JOREK) residuals
 *   residual_continuity / residual_temperature          Joint/JOREK_residuals_CP.py:210-243
 * for Nt-FASTEST views - the layout the script holds: vars[BS,F,Nx,Ny,Nt] dense, each field its permute(0,3,1,2) view.
 * One entry evaluates, in ONE launch per output group, the gradient of <gg, r> with respect to the fields r reads.
 *
 * Notation.  D(f)(x) = sum_k w_k f(x+k) with zero padding, D^T the same star with mirrored taps;
 *   X(f) = D_R f D_Z phi - D_R phi D_Z f,   Y(f) = D_RR f + (1/R) D_R f + D_ZZ f,   h = gg R,
 *   gg = m ? host_scale * (*dev_scale) * g : 0  (m: the cells PRE_VJP_CROP keeps),
 *   J(f; s) = D_R^T(h s D_Z f) - D_Z^T(h s D_R f)  (s = 1 where it is left out),
 *   Yt = D_RR^T gg + (1/R) D_R^T gg + D_ZZ^T gg.
 * eq 0, continuity:   r = a0 D_t rho - a1 R X(rho) - a2 rho D_Z phi - a3 Y(rho)
 *     d rho = a0 D_t^T gg - a1 J(phi) - a2 gg D_Z phi - a3 Yt
 *     d phi = a1 J(rho) - a2 D_Z^T(gg rho)
 * eq 1, temperature:  r = T D_t rho + rho D_t T - rho R X(T) + T R X(rho) + a0 rho T D_Z phi + a3 Y(T)
 *     d rho = D_t^T(gg T) + gg D_t T - h X(T) + J(phi; T) + a0 gg T D_Z phi
 *     d T   = gg D_t rho + D_t^T(gg rho) - J(phi; rho) + h X(rho) + a0 gg rho D_Z phi + a3 Yt
 *     d phi = J(T; rho) - J(rho; T) + a0 D_Z^T(gg rho T)
 * R is a grid: it has no gradient.  coef = (a0, a1, a2, a3), the four scalars of pre_residual_jorek_f32 (continuity:
 * (1, 1, 2, D) or the script's folded norms; temperature: (2 gamma, 0, 0, K)).
 *
 * Arguments, as pre_screenjorek_flat_f32 takes them (cp_pre_screenjorek.h) with the gradient plumbing of cp_pre_vjpflatmhd.h:
 *   - fields {rho, phi, T} and out {d rho, d phi, d T} on the caller's LOGICAL extents B, T, X, Y; for eq 0 fields[2] and
 *     out[2] are ignored (not read, not checked, not written: the caller zeroes that slot);
 *   - Rb: the radius as a view that repeats its row along Y: strides (sB, sT, sX, sY) = (0, 1, 0, T) over a [Y][T] array
 *     (the stride of an axis of extent 1 is not looked at); another view of it is PRE_E_UNSUPPORTED;
 *   - K_t, K_R, K_Z, K_RR, K_ZZ: host, dense 3x3x3 on (T, X, Y); coef: host;
 *   - g is read as stored; mask and scale are applied on load, by a select per logical cell; dev_scale is a DEVICE pointer
 *     or NULL and is never read on the host;
 *   - accepted layout, that of cp_pre_vjpflat.h: g, every field read and every output written have sT == 1, sY == T and
 *     sX == Y*T (any sB), (Y * T) % 4 == 0 and T < 96; everything else is PRE_E_UNSUPPORTED, as is any flag but PRE_VJP_CROP;
 *   - PRE_E_NULL for a null pointer or an empty extent; PRE_E_RANGE for eq outside [0, 1]; PRE_E_SHAPE for an output whose
 *     bounding byte range overlaps that of an input (Rb included), two outputs with one base address, or a merged row
 *     beyond 2^30 cells;
 *   - every refusal is returned before any launch; no atomics: the same views give the same bytes on every run; nothing
 *     allocates, nothing synchronises, all work is enqueued on `stream`.
 *
 * Tap structure.  The gradient at a cell reads phi at the four corners of the (R, Z) plane (D_R^T of a field that holds
 * D_Z phi).  The kernels are built for the tap structure the reference constructs - D_t, D_Z and D_ZZ with taps along Nt
 * only, D_R and D_RR along Nx only - in which no operator has a tap along Ny, the axis R varies on: R is read at its
 * centre value.  Everything else - D_Z / D_ZZ along Ny (y_axis_fix), general stars, weight off the 7-point star - is
 * PRE_E_UNSUPPORTED; pre_vjpjorek_supported says so without any views.
 */
#ifndef CP_PRE_VJPJOREK_H
#define CP_PRE_VJPJOREK_H

#include <stdint.h>

#include "cp_pre_vjp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_VJPJOREK_ABI_VERSION 1
int pre_vjpjorek_abi_version(void);  /* == PRE_VJPJOREK_ABI_VERSION */

/* PRE_OK if equation `eq` (0 continuity, 1 temperature) has an instantiation for the tap structure of these kernels,
 * PRE_E_UNSUPPORTED if not (or weight off the star), PRE_E_RANGE for another eq, PRE_E_NULL.  Host only. */
int pre_vjpjorek_supported(int eq, const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ);

int pre_vjpjorek_flat_f32(int eq, const pre_field_t *g, const pre_field_t fields[3], const pre_field_t *Rb, const pre_out_t out[3],
                          const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                          const float coef[4], float host_scale, const float *dev_scale /*device, or NULL*/,
                          int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_VJPJOREK_H */
