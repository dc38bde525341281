/* cp_pre_screen1dpair.h - C ABI of libcp_pre_screen1dpair.so: the calibrated-set screen of cp_pre_screen1d.h (the 1-D
 * residuals on [B,Nt,Nx] fields, a sample one [Nt,Nx] plane) for the data-driven scores of cp_pre_pair.h - the question
 * the Joint/ scripts of the 1-D surrogates ask of their held-out pairs after calibrating on r(y) - r(y_hat):
 *   Joint/Burgers_Residuals_CP.py:217-220, 250-259, Joint/Advection_Residuals_CP.py, and the <kind>_AL_Joint.py loops of
 *   Active_Learning that hold pred.permute(0,1,3,2)[:,0].
 * Each entry is ONE streaming pass over BOTH field sets of a [B,T,X] batch (T = Nt, X = Nx) that evaluates the two
 * residuals in registers and reduces their difference, per sample, to
 *   d             = fl(fl(r(a)) - fl(r(b)))     each half rounded to fp32 before the subtraction, as libcp_pre_pair.so does
 *   score[b]      = max over the counted cells of |d| / m
 *   count[k][b]   = number of counted cells with |d| <= fl(q[k] * m)   (k < nk <= PRE_SCREEN_MAX_LEVELS)
 * Neither residual nor d is written.
 *
 * Semantics: this is the one-sided test on the difference - what pre_pair_*_f32, the joint score and pre_cov_levels_f32
 * give in three passes.  It is NOT the reference's two-sided form c - hw <= y <= c + hw on the two residual arrays: the two
 * can differ in a cell that sits within rounding of the band's edge.
 *
 * Conventions:
 *   - set `a` is the truth (r(y)), set `b` the prediction (r(y_hat)); `strides_a` / `strides_b` are their element strides
 *     on (B, Nt, Nx): each set has its own sample and row pitch, and the two may be the same memory (then every score is +0
 *     and every cell with q[k] * m >= 0 is inside);
 *   - both sets need their unit stride on the SAME axis, Nx (strides[2] == 1) or Nt (strides[1] == 1), and the modulation
 *     its unit stride on that axis too;
 *   - each entry takes the arguments of its single-set twin (pre_screen1d_*_f32) with the twin's field replaced by the two
 *     sets, `a` first; pre_screen_t is read as cp_pre_screen1d.h reads it (`ct` the Nt crop, `cx` the Nx crop, `cy` 0;
 *     `mT` / `mX` the modulation's Nt / Nx strides);
 *   - everything else - accumulation by integer maximum and integer adds, the crop by select, the guarded divide, sticky
 *     NaN, the non-finite contract, hw = q[k] * m as one fp32 multiplication, `q` on the device - is cp_pre_screen1d.h's
 *     and holds for both sets;
 *   - PRE_E_UNSUPPORTED before any launch for: sets whose unit-stride axes differ (or differ from the modulation's, or
 *     that have none), a contiguous-axis length that is no multiple of 4, a tap or an operator weight off the 5-point star
 *     of the (Nt, Nx) plane, any flag (the caller takes its three-pass route);
 *   - PRE_E_NULL for a null pointer (of either set), an empty extent or count_ld < B, PRE_E_RANGE for nk outside
 *     [1, PRE_SCREEN_MAX_LEVELS], a negative crop or cy != 0, PRE_E_SHAPE for T*X >= 2^32 (the counts are 32-bit), a
 *     contiguous axis beyond 2^28 cells or a tap offset beyond +-3;
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`.
 */
#ifndef CP_PRE_SCREEN1DPAIR_H
#define CP_PRE_SCREEN1DPAIR_H

#include <stdint.h>

#include "cp_pre_screen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SCREEN1DPAIR_ABI_VERSION 1
int pre_screen1dpair_abi_version(void);  /* == PRE_SCREEN1DPAIR_ABI_VERSION */

/* d = S(a) - S(b), S a tap list (host arrays, 2 offsets per tap: Nt, Nx) as pre_screen1d_stencil2d_f32 takes it: any
 * ConvOperator of Utils/ConvOps_1d.py:150 and the advection residual on truth and prediction,
 * Joint/Advection_Residuals_CP.py:156-164. */
int pre_screen1dpair_stencil2d_f32(const float *a, const int64_t strides_a[3], const float *b, const int64_t strides_b[3],
                                   const float *tap_w /*host*/, const int32_t *tap_off /*host, 2*ntaps*/, int ntaps,
                                   const pre_screen_t *s,
                                   int64_t B, int64_t T, int64_t X, int flags, void *stream);

/* d = the Burgers residual of pre_screen1d_burgers_f32 on a less that on b (K_t, K_x, K_xx dense 3x3 host kernels on
 * (Nt, Nx)), Joint/Burgers_Residuals_CP.py:217-220, 250-259. */
int pre_screen1dpair_burgers_f32(const float *a, const int64_t strides_a[3], const float *b, const int64_t strides_b[3],
                                 const float *K_t, const float *K_x, const float *K_xx,
                                 float dx, float dt, float nu, float c3, const pre_screen_t *s,
                                 int64_t B, int64_t T, int64_t X, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_SCREEN1DPAIR_H */
