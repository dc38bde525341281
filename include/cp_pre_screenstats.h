/* cp_pre_screenstats.h - C ABI of libcp_pre_screenstats.so: per-sample statistics of a residual in one streaming launch
 * that stores no residual.
 *
 * The active-learning loops order their candidate predictions by a per-sample magnitude of the residual (acquisition 'PRE'):
 *   torch.sort(torch.mean(torch.abs(pred_residual), axis=...))   Active_Learning/Wave_AL_Joint.py:403-408
 *                                                                Active_Learning/Advection_AL_Joint.py:340-345
 *   torch.sort(torch.mean(pred_residual, axis=...))              Active_Learning/Burgers_AL_Joint.py:340-345
 * and the per-sample mean of r^2 is the per-sample term of PI_loss.  Each entry below is ONE streaming pass over the fields
 * of a batch that evaluates the residual r in registers (the marches and functors of cp_pre_screen.h, cp_pre_screenflat.h
 * and cp_pre_screen1d.h, unchanged) and reduces it, per sample b, over the counted cells to
 *   sums[0][b] += sum r      sums[1][b] += sum |r|      sums[2][b] += sum r^2      max_abs[b] = max(max_abs[b], max |r|)
 * followed by one tiny launch on the same stream that adds the workgroups' partial sums.  The counted cells are
 * t in [ct, T - ct), x in [cx, X - cx), y in [cy, Y - cy) (the 1-D family: cy == 0).
 *
 * Conventions (types, flags, error codes and their order are those of cp_pre_screen.h / cp_pre_screenflat.h /
 * cp_pre_screen1d.h for the three forms):
 *   - `max_abs` is uint32 [B] in memory (read it as float): an unsigned integer maximum of the fp32 bit pattern, NaN sticky
 *     (its pattern lies above +inf), accumulated across calls.  The caller zeroes it before the first slab;
 *   - `sums` is double [3][sum_ld], sum_ld >= B, ADD-accumulated across calls; the caller zeroes it before the first slab.
 *     Every addition is fp64 from the first one: (double) r, its absolute value, its square (exact in fp64).  No
 *     floating-point atomic anywhere: a workgroup stores its three partial sums into its own slot of `workspace`, and the
 *     second launch adds each sample's slots in index order.  The same inputs and the same sequence of calls give the same
 *     bytes on every run.  Slabs of one grid compose to the bits of the whole grid in max_abs, and in the sums to within
 *     fp64 rounding of a different order of the same terms;
 *   - `workspace`: device, `workspace_len` doubles, at least pre_screenstats_workspace_len(form, B, T, X, Y) of them.  Its
 *     contents before a call do not matter (every slot that is read is written first, a workgroup with nothing to count
 *     writes zeros) and mean nothing afterwards.  Calls that share a workspace must be on one stream;
 *   - a cell outside the counted region contributes exactly nothing, whatever it holds (masked by a select): a NaN or inf in
 *     a cropped rim cell, a halo row or a halo plane reaches no result.  A NaN in a counted cell makes the sample's four
 *     statistics NaN;
 *   - PRE_FLAG_HALO_X and PRE_FLAG_INTERIOR_T on the Ny-fastest form, PRE_FLAG_INTERIOR_T on the Nt-fastest form, no flag
 *     on the 1-D form, as in the three headers; other flags: PRE_E_UNSUPPORTED;
 *   - PRE_E_UNSUPPORTED before any launch for everything the three headers decline (operator weight off the star, a layout
 *     the form does not take, widths that are no multiple of 4) and for the instantiations that are not built: the
 *     general-star tap structure of the MHD momentum and energy equations, in both 2-D forms (they do not fit the
 *     register file next to the fp64 accumulators; the tap structures of the reference's operators are built);
 *   - PRE_E_NULL for a null pointer, an empty extent, sum_ld < B or a workspace shorter than the query's answer,
 *     PRE_E_RANGE for a negative crop (the 1-D form: cy != 0) or eq outside [0, 3], PRE_E_SHAPE as in the three headers;
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`.
 */
#ifndef CP_PRE_SCREENSTATS_H
#define CP_PRE_SCREENSTATS_H

#include <stdint.h>

#include "cp_pre_screen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SCREENSTATS_ABI_VERSION 1
int pre_screenstats_abi_version(void);  /* == PRE_SCREENSTATS_ABI_VERSION */

/* the three forms, for the workspace query */
#define PRE_SCREENSTATS_FORM_NY 0     /* Ny-fastest fields [B,T,X,Y]: pre_screenstats_*_f32 */
#define PRE_SCREENSTATS_FORM_FLAT 1   /* Nt-fastest fields, memory [B,X,Y,T]: pre_screenstats_flat_*_f32 */
#define PRE_SCREENSTATS_FORM_ROWS 2   /* the 1-D family [B,T,X] in either layout (Y is ignored): pre_screenstats_rows_*_f32 */

typedef struct {
    int ct, cx, cy;            /* cells per side left out of the counted region (logical axes) */
    uint32_t *max_abs;         /* device [B]: bits of max |r|, max-accumulated */
    double *sums;              /* device [3][sum_ld]: sum r, sum |r|, sum r^2, add-accumulated */
    int64_t sum_ld;
    double *workspace;         /* device, workspace_len doubles */
    int64_t workspace_len;
} pre_screenstats_t;

/* Host only (no device is touched): the doubles `workspace` must hold for a call of `form` on (B, T, X, Y); an upper bound
 * of 3 x the workgroups any entry of that form launches.  0 for a form or an extent out of range. */
int64_t pre_screenstats_workspace_len(int form, int64_t B, int64_t T, int64_t X, int64_t Y);

/* Ny-fastest fields: the residuals of pre_screen_stencil3d_f32, pre_screen_linear2_f32, pre_screen_ns_momentum_f32 and
 * pre_screen_mhd_f32 (all four equations), argument for argument. */
int pre_screenstats_stencil3d_f32(const pre_field_t *f, const float *tap_w /*host*/, const int32_t *tap_off /*host, 3*ntaps*/,
                                  int ntaps, const pre_screenstats_t *s,
                                  int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screenstats_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                                const pre_screenstats_t *s,
                                int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screenstats_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                    const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                    float dt, float dx, float dy, float nu, const pre_screenstats_t *s,
                                    int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screenstats_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y,
                            double gamma, const pre_screenstats_t *s,
                            int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* Nt-fastest fields (the accepted layout of cp_pre_screenflat.h; shapes and crops on the logical [B,T,X,Y]). */
int pre_screenstats_flat_stencil3d_f32(const pre_field_t *f, const float *tap_w /*host*/, const int32_t *tap_off /*host*/,
                                       int ntaps, const pre_screenstats_t *s,
                                       int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screenstats_flat_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b,
                                     float ratio, const pre_screenstats_t *s,
                                     int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screenstats_flat_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                         const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                         float dt, float dx, float dy, float nu, const pre_screenstats_t *s,
                                         int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screenstats_flat_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y,
                                 double gamma, const pre_screenstats_t *s,
                                 int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* The 1-D family on [B,T,X] (T = Nt, X = Nx), Nx-fastest or Nt-fastest: the residuals of pre_screen1d_stencil2d_f32 and
 * pre_screen1d_burgers_f32, argument for argument; `ct` is the Nt crop, `cx` the Nx crop, `cy` must be 0. */
int pre_screenstats_rows_stencil2d_f32(const float *u, const int64_t strides[3], const float *tap_w /*host*/,
                                       const int32_t *tap_off /*host, 2*ntaps*/, int ntaps, const pre_screenstats_t *s,
                                       int64_t B, int64_t T, int64_t X, int flags, void *stream);
int pre_screenstats_rows_burgers_f32(const float *u, const int64_t strides[3], const float *K_t, const float *K_x,
                                     const float *K_xx, float dx, float dt, float nu, float c3, const pre_screenstats_t *s,
                                     int64_t B, int64_t T, int64_t X, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_SCREENSTATS_H */
