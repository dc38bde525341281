/* cp_pre_screencells.h - C ABI of libcp_pre_screencells.so: the calibrated-set screens of cp_pre_screen.h (Ny-fastest
 * fields) and cp_pre_screenflat.h (Nt-fastest fields) against PER-CELL sets at up to 16 levels in one launch.
 *
 * The marginal scripts of the reference calibrate a quantile per cell at ten alphas and then ask, for each alpha, whether
 * the residual of every held-out prediction lies inside +-qhat[k][cell]:
 *   Marginal/NS_Residuals_CP.py:307-337, Marginal/MHD_Residuals_CP.py:408-418, Marginal/Wave_Residuals_CP.py:284-288
 * Each entry below is ONE streaming pass over the fields of a [B,T,X,Y] batch that evaluates the residual r in registers
 * (the marches and functors of the pre_screen_*_f32 / pre_screenflat_*_f32 entries, unchanged) and reduces it, per sample, to
 *   score[b]      = max over the counted cells of |r| / m                      (m == 1 without a modulation)
 *   count[k][b]   = number of counted cells with |r| <= hw,  hw = levels[k][cell]        without a modulation,
 *                                                            hw = fl(levels[k][cell] * m[cell])   with one
 * The residual is never written.  count is what pre_cov_levels_f32 counts with q_ld != 0, per sample.
 *
 * Everything cp_pre_screen.h / cp_pre_screenflat.h say of their entries - accumulation by integer atomics, the crop, the
 * flags, the non-finite contract, the accepted layouts, the error codes - holds for the entries of the same form here.
 * What differs is the sets:
 *   - `levels`: DEVICE pointer to nk level fields [T,X,Y], shared by all samples, level k at levels + k * lK.  In the
 *     Ny-fastest form a level field has plane and row strides lT, lX and unit stride on Y, as the modulation of
 *     pre_screen_t; in the flat form it needs lT == 1 and lY == T (any lX), as the modulation of pre_screenflat_t, else
 *     PRE_E_UNSUPPORTED.  lK is any non-negative stride;
 *   - a level value outside the counted region is never used (its rim may hold anything; along the unit-stride axis a rim
 *     cell is read with the quad it shares with counted cells and masked).  Inside the region a NaN level or a NaN r puts
 *     the cell outside at that level, a negative level puts it outside, +inf puts it inside for every non-NaN r;
 *   - block order: the samples are taken in groups of pre_screencells_sample_group(), the sample of a group the fastest
 *     block index, so that the workgroups one XCD runs together read the same level quads.  It is speed only: every
 *     (sample, tile, segment) is visited exactly once for every B.
 */
#ifndef CP_PRE_SCREENCELLS_H
#define CP_PRE_SCREENCELLS_H

#include <stdint.h>

#include "cp_pre_screenflat.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SCREENCELLS_ABI_VERSION 1
int pre_screencells_abi_version(void);   /* == PRE_SCREENCELLS_ABI_VERSION */
int pre_screencells_sample_group(void);  /* samples per group of the block order (>= 1), a constant of the build */

/* pre_screen_t with level fields in place of q */
typedef struct {
    const float *levels;       /* device, nk fields [T,X,Y] */
    int nk;
    int64_t lK, lT, lX;        /* level, plane and row strides in elements (last axis: 1) */
    const float *modulation;   /* device [T,X,Y] or NULL (m == 1) */
    int64_t mT, mX;            /* its plane and row strides in elements (last axis: 1) */
    int ct, cx, cy;            /* cells per side left out of the counted region */
    uint32_t *score;           /* device [B]: bits of max |r|/m, max-accumulated */
    uint32_t *count;           /* device [nk][count_ld]: cells inside, add-accumulated */
    int64_t count_ld;
} pre_screencells_t;

/* pre_screenflat_t with level fields in place of q: the unit-stride axis is T */
typedef struct {
    const float *levels;       /* device, nk fields [T,X,Y] with memory [X,Y,T] */
    int nk;
    int64_t lK, lT, lX, lY;    /* level stride, then the strides on the logical axes: lT == 1, lY == T */
    const float *modulation;   /* device [T,X,Y] or NULL (m == 1) */
    int64_t mT, mX, mY;        /* its strides in elements on the logical axes: mT == 1, mY == T */
    int ct, cx, cy;            /* cells per side left out of the counted region (logical axes) */
    uint32_t *score;
    uint32_t *count;
    int64_t count_ld;
} pre_screencellsflat_t;

/* Ny-fastest fields: the arguments of pre_screen_*_f32 with pre_screencells_t in place of pre_screen_t */
int pre_screencells_stencil3d_f32(const pre_field_t *f, const float *tap_w /*host*/, const int32_t *tap_off /*host, 3*ntaps*/,
                                  int ntaps, const pre_screencells_t *s,
                                  int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screencells_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                                const pre_screencells_t *s,
                                int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screencells_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                    const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                    float dt, float dx, float dy, float nu, const pre_screencells_t *s,
                                    int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screencells_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y,
                            double gamma, const pre_screencells_t *s,
                            int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* Nt-fastest fields (pred.permute(0,1,4,2,3), what the NS and MHD scripts pass): the arguments of pre_screenflat_*_f32 */
int pre_screencells_flat_stencil3d_f32(const pre_field_t *f, const float *tap_w /*host*/, const int32_t *tap_off /*host*/,
                                       int ntaps, const pre_screencellsflat_t *s,
                                       int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screencells_flat_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b,
                                     float ratio, const pre_screencellsflat_t *s,
                                     int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screencells_flat_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                         const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                         float dt, float dx, float dy, float nu, const pre_screencellsflat_t *s,
                                         int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);
int pre_screencells_flat_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y,
                                 double gamma, const pre_screencellsflat_t *s,
                                 int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_SCREENCELLS_H */
