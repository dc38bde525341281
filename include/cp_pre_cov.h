/* cp_pre_cov.h - C ABI of libcp_pre_cov.so: empirical coverage at several calibration levels in one pass over the test
 * residual (cp_pre_amd.inductive_cp.emp_cov_levels / emp_cov_joint_levels, cp_pre_amd.pipeline.CoverageLevels).
 *
 * The reference ends every calibration script with a loop over alpha levels that builds a prediction set per level and
 * measures its coverage (Marginal/NS_Residuals_CP.py:308-312, 333-337; Joint/MHD_Residuals_CP.py:390-394, 416-420).  One
 * launch here reads the test residual once for up to PRE_COV_MAX_LEVELS levels.
 *
 * Operands.  y (the test residual) and the optional centre c are n samples of A x B x C cells, addressed where they lie:
 * cell (a, b, x) of sample s is ptr[s*sN + a*sA + b*sB + x] (element strides; the innermost axis is dense).  The flat cell
 * index is j = (a*B + b)*C + x, the order of the per-cell operands below.
 * Half-widths, fp32 (the reference's operation order; the library is built without fma contraction):
 *   hw = q[k] (q_ld == 0: one scalar per level, the joint q-hat) or q[k*q_ld + j] (per level and cell, the marginal one),
 *   hw = hw * m[j] when the modulation m (per cell) is given;
 *   lo = c - hw, hi = c + hw (no centre: lo = -hw, hi = hw);  the cell is inside iff y >= lo && y <= hi (IEEE: NaN is
 *   outside, a value on a bound inside).
 * Outputs accumulate, so slabs of cells and of samples compose (the caller clears them once):
 *   count != NULL (marginal): count[k] += #(sample, cell) inside at level k;
 *   inside != NULL (joint):   inside[k*inside_ld + s] = 0 where any cell of sample s is outside at level k (0 / 1 bytes).
 * Exactly one of count / inside is given.  nk > PRE_COV_MAX_LEVELS is split into launches of at most that many levels.
 *
 * Every call is asynchronous on the given HIP stream and never synchronises.  Return codes: 0 ok; < 0 as in cp_pre_hip.h
 * (PRE_E_*); > 0 a hipError_t.
 */
#ifndef CP_PRE_COV_H
#define CP_PRE_COV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_COV_ABI_VERSION 1
#define PRE_COV_MAX_LEVELS 16    /* levels per launch */

int pre_cov_abi_version(void);

int pre_cov_levels_f32(const float *y, int64_t y_sN, int64_t y_sA, int64_t y_sB,
                       const float *c, int64_t c_sN, int64_t c_sA, int64_t c_sB,
                       int64_t n, int64_t A, int64_t B, int64_t C,
                       const float *q, int64_t q_ld, const float *m, int nk,
                       uint64_t *count, uint8_t *inside, int64_t inside_ld, void *stream);

#ifdef __cplusplus
}
#endif
#endif
