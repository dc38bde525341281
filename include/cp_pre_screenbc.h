/* cp_pre_screenbc.h - C ABI of libcp_pre_screenbc.so: the calibrated-set screen (cp_pre_screen.h) and the per-sample
 * statistics (cp_pre_screenstats.h) of the 2-D residuals under boundary conditions on the x-y rim (cp_pre_bcres.h), in one
 * streaming launch that stores no residual.
 *
 * The screened quantity is the residual of cp_pre_bcres.h,
 *     r_bc(fields) = r_zero_pad( pad(f) for f in fields )[..., :, 1:-1, 1:-1],
 * valid on the whole x-y plane; the time axis keeps its zero padding.  What is done with it is what the zero-pad entries do:
 *   pre_screenbc_*_f32        score[b] = max |r| / m, count[k][b] += #{|r| <= q_k m}      (cp_pre_screen.h, argument for argument)
 *   pre_screenbc_stats_*_f32  sum r, sum |r|, sum r^2 in fp64 and max |r|                  (cp_pre_screenstats.h, likewise)
 * over the counted cells t in [ct, T - ct), x in [cx, X - cx), y in [cy, Y - cy); a caller that counts the whole plane passes
 * cx == cy == 0.  The march and the functors are those of the zero-pad screens, compiled with the same flags: a cell whose
 * star stays inside the grid gets the same bits.
 *
 * Conventions (types, flags and error codes are those of cp_pre_hip.h; the descriptors those of cp_pre_screen.h and
 * cp_pre_screenstats.h with their accumulation rules; `bc` is the pre_bc_t of cp_pre_bcres.h, host memory, one condition per
 * side for every field):
 *   - Ny-fastest fields only: every view needs unit stride on Ny and Y % 4 == 0, the conditions are tied to the axes and
 *     nothing is relabelled;
 *   - flags: PRE_FLAG_INTERIOR_T keeps its meaning; PRE_FLAG_HALO_X is PRE_E_UNSUPPORTED (an x-slab has no rim of its own);
 *   - checked in this order, all before any launch: the kernels' and `bc`'s nulls (PRE_E_NULL), eq (PRE_E_RANGE), what the
 *     zero-pad entry checks of its descriptor and views (PRE_E_NULL / PRE_E_RANGE / PRE_E_SHAPE, then PRE_E_UNSUPPORTED for
 *     the layout), PRE_FLAG_HALO_X (PRE_E_UNSUPPORTED), an unknown mode or X < 2 / Y < 2 under a PRE_BC_REFLECT side and
 *     in-plane offsets beyond 32 bits (PRE_E_RANGE), operator weight off the 7-point star and a tap structure that is not
 *     built (PRE_E_UNSUPPORTED);
 *   - built: every functor in the reference's tap structure and the y-fixed one, for both the levels and the statistics;
 *     the general star too, except for MHD momentum and MHD energy (eq 1, 2), whose six views with a second edge scalar per
 *     field do not fit the register file.  No instantiation that is built uses scratch (profiles/screenbc/resources.txt);
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`.
 */
#ifndef CP_PRE_SCREENBC_H
#define CP_PRE_SCREENBC_H

#include <stdint.h>

#include "cp_pre_bcres.h"
#include "cp_pre_screen.h"
#include "cp_pre_screenstats.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SCREENBC_ABI_VERSION 1
int pre_screenbc_abi_version(void);     /* == PRE_SCREENBC_ABI_VERSION */

/* Host only: the doubles pre_screenstats_t::workspace must hold for a pre_screenbc_stats_*_f32 call on (B, T, X, Y); the
 * answer of pre_screenstats_workspace_len(PRE_SCREENSTATS_FORM_NY, ...).  0 for an extent out of range. */
int64_t pre_screenbc_stats_workspace_len(int64_t B, int64_t T, int64_t X, int64_t Y);

/* the screens of cp_pre_screen.h on the residual under `bc` */
int pre_screenbc_stencil3d_f32(const pre_field_t *f, const float *tap_w /*host*/, const int32_t *tap_off /*host, 3*ntaps*/,
                               int ntaps, const pre_screen_t *s, const pre_bc_t *bc,
                               int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screenbc_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                             const pre_screen_t *s, const pre_bc_t *bc,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screenbc_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                 const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                 float dt, float dx, float dy, float nu, const pre_screen_t *s, const pre_bc_t *bc,
                                 int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screenbc_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y,
                         double gamma, const pre_screen_t *s, const pre_bc_t *bc,
                         int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* the statistics of cp_pre_screenstats.h (Ny-fastest form) on the residual under `bc` */
int pre_screenbc_stats_stencil3d_f32(const pre_field_t *f, const float *tap_w /*host*/, const int32_t *tap_off /*host*/,
                                     int ntaps, const pre_screenstats_t *s, const pre_bc_t *bc,
                                     int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screenbc_stats_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b,
                                   float ratio, const pre_screenstats_t *s, const pre_bc_t *bc,
                                   int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screenbc_stats_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                       const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                       float dt, float dx, float dy, float nu, const pre_screenstats_t *s, const pre_bc_t *bc,
                                       int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screenbc_stats_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y,
                               double gamma, const pre_screenstats_t *s, const pre_bc_t *bc,
                               int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_SCREENBC_H */
