/* cp_pre_screenflat.h - C ABI of libcp_pre_screenflat.so: the calibrated-set screen of cp_pre_screen.h for Nt-FASTEST views
 * of the 2-D residuals - the layout the reference's own scripts pass:
 *   residual_momentum(pred.permute(0,1,4,2,3)) followed by emp_cov_joint / filter_sims_joint
 *                                                     Joint/NS_Residuals_CP.py:282-305,328-357
 *                                                     Joint/MHD_Residuals_CP.py:326-346,409-410
 * Each pre_screenflat_*_f32 entry is ONE streaming pass over the fields of a [B,T,X,Y] batch whose memory is [B,X,Y,T]
 * (the surrogate's native output) that evaluates the residual r in registers (the functors of the pre_residual_*_f32
 * entries in their flat form, unchanged) and reduces it, per sample, to
 *   score[b]      = max over the counted cells of |r| / m          (ncf_metric_joint, Joint/NS_Residuals_CP.py:318-320)
 *   count[k][b]   = number of counted cells with |r| <= q[k] * m   (k < nk <= PRE_SCREEN_MAX_LEVELS)
 * The residual is never written.  Shapes and crops are the caller's LOGICAL [B,T,X,Y]: the counted cells are t in
 * [ct, T - ct), x in [cx, X - cx), y in [cy, Y - cy); the library relabels the axes (it marches over X and merges Y and T
 * into one row of Y*T cells).
 *
 * Conventions are those of cp_pre_screen.h (types, flags, error codes of cp_pre_hip.h):
 *   - results are ACCUMULATED: score by an unsigned integer maximum of the fp32 bit pattern (NaN lies above +inf), count
 *     by integer adds.  The caller zeroes both buffers before the first call; batch slabs and repeated calls then compose
 *     exactly, in any order.  `score` is uint32 [B], `count` uint32 [nk][count_ld], count_ld >= B.  Integer atomics only: the
 *     same input gives the same bytes on every run;
 *   - the non-finite contract: a cell outside the counted region contributes nothing, whatever it holds (masked by a
 *     select).  Inside it, NaN r or m (and 0/0) make the score NaN and the cell outside at every level; m == 0 with
 *     r != 0 gives an inf score and the cell outside;
 *   - hw = q[k] * m is one fp32 multiplication (no fma), the inside test |r| <= hw: what libcp_pre_cov.so computes;
 *   - `q`: DEVICE pointer to nk fp32 levels;
 *   - accepted layout: every field view has sT == 1 and sY == T (any sX, sB), Y > 1, (Y * T) % 4 == 0 and
 *     T < 96 - the condition under which pre_residual_*_f32 takes its flat form; `modulation` m[T,X,Y] is shared by all
 *     samples and needs mT == 1 and mY == T (any mX); NULL means m == 1.  Its values outside the counted region are never
 *     used;
 *   - PRE_FLAG_INTERIOR_T: logical planes t = 0 and t = T - 1 are not counted (as if ct >= 1);
 *   - PRE_E_UNSUPPORTED before any launch for: everything outside the accepted layout - a unit-stride last axis included:
 *     that is libcp_pre_screen.so's -, operator weight off the 7-point star, PRE_FLAG_HALO_X (the flat form pads the
 *     marched axis' neighbours in the row with zeros) and every other flag, and the one instantiation that is not built
 *     (the general-star tap structure of the MHD momentum equation: it does not fit the register file);
 *   - PRE_E_NULL for a null pointer, an empty extent or count_ld < B, PRE_E_RANGE for nk outside
 *     [1, PRE_SCREEN_MAX_LEVELS], a negative crop or eq outside [0, 3], PRE_E_SHAPE for T*X*Y >= 2^32 (the counts are
 *     32-bit), a merged row beyond 2^30 cells or a tap offset beyond +-3;
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`.
 */
#ifndef CP_PRE_SCREENFLAT_H
#define CP_PRE_SCREENFLAT_H

#include <stdint.h>

#include "cp_pre_screen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SCREENFLAT_ABI_VERSION 1
int pre_screenflat_abi_version(void);  /* == PRE_SCREENFLAT_ABI_VERSION */

/* pre_screen_t with three modulation strides: the unit-stride axis is T */
typedef struct {
    const float *q;            /* device, nk levels */
    int nk;
    const float *modulation;   /* device [T,X,Y] or NULL (m == 1) */
    int64_t mT, mX, mY;        /* its strides in elements on the logical axes: mT == 1, mY == T */
    int ct, cx, cy;            /* cells per side left out of the counted region (logical axes) */
    uint32_t *score;           /* device [B]: bits of max |r|/m, max-accumulated */
    uint32_t *count;           /* device [nk][count_ld]: cells inside, add-accumulated */
    int64_t count_ld;
} pre_screenflat_t;

/* r = S(f), S a tap list (host arrays, 3 offsets per tap on the logical (T,X,Y)) as pre_stencil3d_f32 takes it: the wave
 * residual on u.permute(0,1,4,2,3), Marginal/Wave_Residuals_CP.py:216, screened as Other_UQ/Evaluation/Eval.py:287-288. */
int pre_screenflat_stencil3d_f32(const pre_field_t *f, const float *tap_w /*host*/, const int32_t *tap_off /*host, 3*ntaps*/,
                                 int ntaps, const pre_screenflat_t *s,
                                 int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* r = Ka(f0) + ratio*Kb(f1): NS continuity (Joint/NS_Residuals_CP.py:222-228), MHD gauss. */
int pre_screenflat_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                               const pre_screenflat_t *s,
                               int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* r = the NS momentum residual of pre_residual_ns_momentum_f32 on pred.permute(0,1,4,2,3), screened as
 * Joint/NS_Residuals_CP.py:282-305,328-357 does. */
int pre_screenflat_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                   const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                   float dt, float dx, float dy, float nu, const pre_screenflat_t *s,
                                   int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* r = equation `eq` of pre_residual_mhd_f32 (0 continuity, 1 momentum, 2 energy, 3 induction; fields rho,u,v,p,Bx,By) on
 * the permuted prediction, screened as Joint/MHD_Residuals_CP.py:326-346,409-410 does. */
int pre_screenflat_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y,
                           double gamma, const pre_screenflat_t *s,
                           int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_SCREENFLAT_H */
