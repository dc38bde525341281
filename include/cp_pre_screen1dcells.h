/* cp_pre_screen1dcells.h - C ABI of libcp_pre_screen1dcells.so: the calibrated-set screens of cp_pre_screen1d.h and
 * cp_pre_screen1dpair.h (the 1-D residuals on [B,Nt,Nx] fields, a sample one [Nt,Nx] plane) against PER-CELL sets at up to
 * 16 levels in one launch.
 *
 * The marginal scripts of the 1-D surrogates calibrate a quantile per cell and then keep or reject every candidate by the
 * share of its cells inside +-qhat[k][cell]:
 *   Active_Learning/Advection_AL_Marginal.py:169-198, 290-311   (filter_sims_within_bounds on per-cell bounds, in a loop)
 *   Marginal/Burgers_Residuals_CP.py:274-283, Marginal/Advection_Residuals_CP.py   (pred_residual against +-qhat at ten alphas)
 *   Marginal/Burgers_Residuals_CP.py:249-259                    (|r(y) - r(y_hat)| <= qhat[cell] on held-out pairs)
 * Each entry below is ONE streaming pass over a [B,T,X] batch (T = Nt, X = Nx; two field sets for the pair entries) that
 * evaluates the residual r in registers (the row march and the functors of the pre_screen1d_*_f32 / pre_screen1dpair_*_f32
 * entries, unchanged; for a pair r is d = fl(fl(r(a)) - fl(r(b)))) and reduces it, per sample, to
 *   score[b]      = max over the counted cells of |r| / m                      (m == 1 without a modulation)
 *   count[k][b]   = number of counted cells with |r| <= hw,  hw = levels[k][cell]               without a modulation,
 *                                                            hw = fl(levels[k][cell] * m[cell])  with one
 * The residual is never written.  count is what pre_cov_levels_f32 counts with q_ld != 0, per sample.  For a pair this is the
 * one-sided test on the difference, as cp_pre_screen1dpair.h states it.
 *
 * Everything cp_pre_screen1d.h / cp_pre_screen1dpair.h say of their entries - accumulation by integer atomics (score by an
 * unsigned maximum of the fp32 bits, count by integer adds: repeated calls and row slabs with crops that count every cell
 * once compose to the bits of the whole sample, in any order), the crop (`ct` the Nt crop, `cx` the Nx crop), the
 * non-finite contract, the accepted layouts, the error codes and their order - holds for the entries here.  What differs is
 * the sets:
 *   - `levels`: DEVICE pointer to nk level fields [T,X], shared by all samples, level k at levels + k * lK, with Nt stride
 *     lT and Nx stride lX (elements).  lK >= 0 is any stride (0: every level the same field);
 *   - the fields (every set), the modulation and the levels must have unit stride on the SAME axis, Nx (the reference
 *     layout) or Nt (u.permute(0,1,3,2)[:,0] of the surrogate's native layout), else PRE_E_UNSUPPORTED; a contiguous-axis
 *     length that is no multiple of 4 is PRE_E_UNSUPPORTED, as there.  A negative lK or row stride is PRE_E_SHAPE;
 *   - a level value outside the counted region is never used (its rim may hold anything; along the unit-stride axis a rim
 *     cell is read with the quad it shares with counted cells and masked).  Inside the region a NaN level or a NaN r puts
 *     the cell outside at that level, a negative level puts it outside, +inf puts it inside for every non-NaN r;
 *   - block order: the samples are taken in groups of pre_screen1dcells_sample_group(), the sample of a group the fastest
 *     block index, so that the workgroups one XCD runs together read the same level quads.  It is speed only: every
 *     (sample, chunk, column tile) is visited exactly once for every B, and every group size gives the same bytes.
 */
#ifndef CP_PRE_SCREEN1DCELLS_H
#define CP_PRE_SCREEN1DCELLS_H

#include <stdint.h>

#include "cp_pre_screen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SCREEN1DCELLS_ABI_VERSION 1
int pre_screen1dcells_abi_version(void);   /* == PRE_SCREEN1DCELLS_ABI_VERSION */
int pre_screen1dcells_sample_group(void);  /* samples per group of the block order (>= 1), a constant of the build */

/* pre_screen_t as cp_pre_screen1d.h reads it, with level fields in place of q */
typedef struct {
    const float *levels;       /* device, nk fields [T,X] */
    int nk;
    int64_t lK, lT, lX;        /* level, Nt and Nx strides in elements (one of lT, lX is 1) */
    const float *modulation;   /* device [T,X] or NULL (m == 1) */
    int64_t mT, mX;            /* its Nt and Nx strides in elements */
    int ct, cx;                /* rows / columns per side left out of the counted region: t in [ct, T-ct), x in [cx, X-cx) */
    uint32_t *score;           /* device [B]: bits of max |r|/m, max-accumulated */
    uint32_t *count;           /* device [nk][count_ld]: cells inside, add-accumulated */
    int64_t count_ld;
} pre_screen1dcells_t;

/* the arguments of pre_screen1d_stencil2d_f32 / pre_screen1d_burgers_f32 with pre_screen1dcells_t in place of pre_screen_t */
int pre_screen1dcells_stencil2d_f32(const float *u, const int64_t strides[3], const float *tap_w /*host*/,
                                    const int32_t *tap_off /*host, 2*ntaps*/, int ntaps, const pre_screen1dcells_t *s,
                                    int64_t B, int64_t T, int64_t X, int flags, void *stream);
int pre_screen1dcells_burgers_f32(const float *u, const int64_t strides[3], const float *K_t, const float *K_x,
                                  const float *K_xx, float dx, float dt, float nu, float c3, const pre_screen1dcells_t *s,
                                  int64_t B, int64_t T, int64_t X, int flags, void *stream);

/* the arguments of pre_screen1dpair_stencil2d_f32 / pre_screen1dpair_burgers_f32 (set `a` the truth, `b` the prediction,
 * each with its own pitches; a == b gives score +0 and every cell inside at every non-negative, non-NaN level) */
int pre_screen1dcells_pair_stencil2d_f32(const float *a, const int64_t strides_a[3], const float *b, const int64_t strides_b[3],
                                         const float *tap_w /*host*/, const int32_t *tap_off /*host, 2*ntaps*/, int ntaps,
                                         const pre_screen1dcells_t *s,
                                         int64_t B, int64_t T, int64_t X, int flags, void *stream);
int pre_screen1dcells_pair_burgers_f32(const float *a, const int64_t strides_a[3], const float *b, const int64_t strides_b[3],
                                       const float *K_t, const float *K_x, const float *K_xx,
                                       float dx, float dt, float nu, float c3, const pre_screen1dcells_t *s,
                                       int64_t B, int64_t T, int64_t X, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_SCREEN1DCELLS_H */
