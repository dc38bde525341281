/* cp_pre_bounds.h - C ABI of libcp_pre_bounds.so: bounds on the solution u by sample acceptance
 * (cp_pre_amd.sample_bounds: sample_envelope, sample_bounds, SampleBounds).
 *
 * The reference's inverse-sampling recipe (Tests/test_advection_inv_sampling_marginal.py:312-359, 363-387, 476-491;
 * Active_Learning/Advection_AL_Marginal.py:169-198): keep the candidate fields u_s whose residual lies inside the
 * calibrated set and report the per-cell envelope (min, max) of the kept ones.  One launch serves up to
 * PRE_BOUNDS_MAX_LEVELS levels and reads u (and r) once; more levels are split into launches by the library.
 *
 * Operands (the cp_pre_cov.h convention).  u, r and the centre c are n samples of A x B x C cells, addressed where they lie:
 * cell (a, b, x) of sample s is ptr[s*sN + a*sA + b*sB + x] (element strides; the innermost axis is dense).  The flat cell
 * index is j = (a*B + b)*C + x, the order of every per-cell operand and result below.  A sample stride of 0 broadcasts.
 *
 * Results accumulate, so that slabs of samples compose; the caller initialises lo = +inf, hi = -inf, counts = 0 once.
 * Semantics (every result is exact: min / max round nothing):
 *   - NaN in u: a NaN in a counted sample makes that cell's bound NaN (numpy's np.min / np.max propagate it; the kernels
 *     use the NaN-propagating v_minimum3 / v_maximum3, so a NaN already in lo / hi also stays);
 *   - no counted sample: lo = +inf, hi = -inf, count 0 (where numpy raises on an empty reduction);
 *   - +0 / -0 and ties: the result compares equal to numpy's (it may differ in the sign of a zero).
 *
 * (a) pre_bounds_envelope_f32: accept[k*accept_ld + s] != 0 marks sample s accepted at level k (uint8, the layout of
 *     pipeline.CoverageLevels.inside).  lo[k*M + j] = min, hi[k*M + j] = max of u[s, j] over the accepted samples;
 *     count[k] += number of accepted samples (int64).  Samples whose accepting levels form a run that starts at the first
 *     level or ends at the last one (nested levels, in either direction) cost one min and one max per element whatever
 *     the number of levels; other samples one per accepting level.
 * (b) pre_bounds_cellwise_f32: cell j of sample s counts at level k iff lo_k(j) <= r[s, j] <= hi_k(j) (NaN outside, a value
 *     on a bound inside).  The bounds, fp32, in the coverage library's order without fma contraction:
 *       hw = q[k] (q_ld == 0) or q[k*q_ld + j];  hw = hw * m[j] when m is given;  lo = c[j] - hw, hi = c[j] + hw (no
 *       centre: -hw, hw);
 *     or given outright (blo / bhi [k*M + j], q, m and c NULL: float64 bounds rounded outwards-in by the caller).
 *     lo / hi[k*M + j] over the counting samples, count[k*M + j] += their number (int32).  r and u share A, B, C.
 * (c) pre_bounds_rowcount_f32: counts[k*counts_ld + s] += number of cells of sample s inside at level k (int32), the
 *     bounds built as in cp_pre_cov.h (q, q_ld, m; the centre c is strided like r, sample stride 0 = one per cell): the
 *     multi-level form of pre_cov_rowcount_f32.
 *
 * Tall inputs (few cells, many samples) split the samples over workgroups; each (split, row of the workgroup) writes
 * partial bounds to the caller's workspace, and a second launch merges them into lo / hi / count.  pre_bounds_*_workspace
 * gives its size in bytes for a shape (0 when the shape needs none); the workspace may be reused after the call's stream
 * work is done.  Every call is asynchronous on the given HIP stream and never synchronises.  Return codes: 0 ok; < 0 as
 * in cp_pre_hip.h (PRE_E_*); > 0 a hipError_t.
 */
#ifndef CP_PRE_BOUNDS_H
#define CP_PRE_BOUNDS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_BOUNDS_ABI_VERSION 1
#define PRE_BOUNDS_MAX_LEVELS 16    /* levels per launch */

int pre_bounds_abi_version(void);

int pre_bounds_envelope_workspace(int64_t n, int64_t A, int64_t B, int64_t C, int nk, int64_t *bytes);

int pre_bounds_envelope_f32(const float *u, int64_t u_sN, int64_t u_sA, int64_t u_sB,
                            int64_t n, int64_t A, int64_t B, int64_t C,
                            const uint8_t *accept, int64_t accept_ld, int nk,
                            float *lo, float *hi, int64_t *count, void *work, int64_t work_bytes, void *stream);

int pre_bounds_cellwise_workspace(int64_t n, int64_t A, int64_t B, int64_t C, int nk, int64_t *bytes);

int pre_bounds_cellwise_f32(const float *u, int64_t u_sN, int64_t u_sA, int64_t u_sB,
                            const float *r, int64_t r_sN, int64_t r_sA, int64_t r_sB,
                            int64_t n, int64_t A, int64_t B, int64_t C,
                            const float *q, int64_t q_ld, const float *m, const float *c,
                            const float *blo, const float *bhi, int nk,
                            float *lo, float *hi, int32_t *count, void *work, int64_t work_bytes, void *stream);

int pre_bounds_rowcount_f32(const float *r, int64_t r_sN, int64_t r_sA, int64_t r_sB,
                            const float *c, int64_t c_sN, int64_t c_sA, int64_t c_sB,
                            int64_t n, int64_t A, int64_t B, int64_t C,
                            const float *q, int64_t q_ld, const float *m, int nk,
                            int32_t *counts, int64_t counts_ld, void *stream);

#ifdef __cplusplus
}
#endif
#endif
