/* cp_pre_screen.h - C ABI of libcp_pre_screen.so: screening predictions against calibrated sets without storing the
 * residual.
 *
 * After a joint calibration the reference asks of every new prediction whether its residual lies inside the set:
 *   filter_sims_joint / emp_cov_joint                 Joint/NS_Residuals_CP.py:328-329,350-352,502-503
 *   the reject-and-resimulate loops                   Active_Learning/Burgers_AL_Joint.py:305-379
 * Each pre_screen_*_f32 entry below is ONE streaming pass over the fields of a [B,T,X,Y] batch that evaluates the
 * residual r in registers (the functors of the pre_residual_*_f32 entries, unchanged) and reduces it, per sample, to
 *   score[b]      = max over the counted cells of |r| / m          (ncf_metric_joint, Joint/NS_Residuals_CP.py:318-320)
 *   count[k][b]   = number of counted cells with |r| <= q[k] * m   (k < nk <= PRE_SCREEN_MAX_LEVELS)
 * The residual is never written.  The counted cells are t in [ct, T - ct), x in [cx, X - cx), y in [cy, Y - cy).
 *
 * Conventions (types, flags, error codes of cp_pre_hip.h):
 *   - results are ACCUMULATED: score by an unsigned integer maximum of the fp32 bit pattern (scores are non-negative, so
 *     the patterns order like the values, and NaN lies above +inf: the propagation of numpy's max), count by integer
 *     adds.  The caller zeroes both buffers before the first slab; x-slabs and t-slabs of one grid then compose to the
 *     bits of the whole grid, in any order.  `score` is uint32 [B] in memory (read it as float), `count` uint32
 *     [nk][count_ld], count_ld >= B.  Integer atomics only: the same input gives the same bytes on every run;
 *   - a cell outside the counted region contributes nothing, whatever it holds (masked by a select): a NaN or inf in a
 *     cropped rim cell or a halo row reaches no result.  Inside it, NaN r or m (and 0/0) make the score NaN and the cell
 *     outside at every level; m == 0 with r != 0 gives an inf score and the cell outside;
 *   - hw = q[k] * m is one fp32 multiplication (no fma), the inside test |r| <= hw: what libcp_pre_cov.so computes;
 *   - `modulation` m[T,X,Y] is shared by all samples: device pointer with its own plane and row strides (elements), unit
 *     stride on its last axis; NULL means m == 1.  Its values outside the counted region are never used;
 *   - `q`: DEVICE pointer to nk fp32 levels (what a calibration left on the device: no host read);
 *   - PRE_FLAG_HALO_X: rows -1 and X of every field view exist and are read as x-neighbours (an x-slab of a larger grid);
 *     PRE_FLAG_INTERIOR_T: planes 0 and T - 1 are neither evaluated nor counted (as if ct >= 1); other flags:
 *     PRE_E_UNSUPPORTED;
 *   - PRE_E_UNSUPPORTED before any launch for: operator weight off the 7-point star, a field or modulation view without
 *     unit stride on its last axis (Nt-fastest views), a row width Y that is no multiple of 4 (the caller takes its
 *     three-pass route; this library is never wrong about a partial quad because it never runs one);
 *   - PRE_E_NULL for a null pointer or an empty extent, PRE_E_RANGE for nk outside [1, PRE_SCREEN_MAX_LEVELS], a negative
 *     crop or eq outside [0, 3], PRE_E_SHAPE for T*X*Y >= 2^32 (the counts are 32-bit) or a plane beyond 32-bit offsets;
 *   - nothing allocates, nothing synchronises, all work is enqueued on `stream`.
 */
#ifndef CP_PRE_SCREEN_H
#define CP_PRE_SCREEN_H

#include <stdint.h>

#include "cp_pre_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SCREEN_MAX_LEVELS 16

#define PRE_SCREEN_ABI_VERSION 1
int pre_screen_abi_version(void);  /* == PRE_SCREEN_ABI_VERSION */

/* what every entry ends with: the sets to screen against and where the verdicts are accumulated */
typedef struct {
    const float *q;            /* device, nk levels */
    int nk;
    const float *modulation;   /* device [T,X,Y] or NULL (m == 1) */
    int64_t mT, mX;            /* its plane and row strides in elements (last axis: 1) */
    int ct, cx, cy;            /* cells per side left out of the counted region */
    uint32_t *score;           /* device [B]: bits of max |r|/m, max-accumulated */
    uint32_t *count;           /* device [nk][count_ld]: cells inside, add-accumulated */
    int64_t count_ld;
} pre_screen_t;

/* r = S(f), S a tap list (host arrays, 3 offsets per tap) as pre_stencil3d_f32 takes it: the wave residual,
 * Other_UQ/Evaluation/PRE_estimations.py:5-21, screened as Other_UQ/Evaluation/Eval.py:287-288 does. */
int pre_screen_stencil3d_f32(const pre_field_t *f, const float *tap_w /*host*/, const int32_t *tap_off /*host, 3*ntaps*/,
                             int ntaps, const pre_screen_t *s,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* r = Ka(f0) + ratio*Kb(f1): NS continuity (Joint/NS_Residuals_CP.py:222-228), MHD gauss. */
int pre_screen_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                           const pre_screen_t *s,
                           int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* r = the NS momentum residual of pre_residual_ns_momentum_f32 (Joint/NS_Residuals_CP.py:231-240), screened as
 * Joint/NS_Residuals_CP.py:328-329,350-352 does. */
int pre_screen_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                               const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                               float dt, float dx, float dy, float nu, const pre_screen_t *s,
                               int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

/* r = equation `eq` of pre_residual_mhd_f32 (0 continuity, 1 momentum, 2 energy, 3 induction; fields rho,u,v,p,Bx,By),
 * screened as Joint/MHD_Residuals_CP.py:409-410 does. */
int pre_screen_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y,
                       double gamma, const pre_screen_t *s,
                       int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_SCREEN_H */
