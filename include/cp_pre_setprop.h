/* cp_pre_setprop.h - C ABI of libcp_pre_setprop.so: PRE set propagation, the step of the reference's Inverted_bounds/SHO.py
 * (set_PRE, 350-407) and Inverse_residuals/Python/pre_set_prop.py (29-91) that pushes a set in residual space (an interval
 * per step) back through the inverse of the ODE operator, giving an interval per step on the solution.  Served by
 * cp_pre_amd.set_prop.
 *
 * Closed form.  The reference's zonotope pipeline (interval DFT, complex product with the inverse spectrum H, inverse
 * interval DFT, real-part interval hull) is linear, so for the residual-space set [c_j - r_j, c_j + r_j], j < N:
 *     centre_k = sum_j c_j * g[(k - j) mod N]
 *     radius_k = sum_j r_j * a[(k - j) mod N]
 *     lower_k = centre_k - radius_k,  upper_k = centre_k + radius_k
 * with g = Re(ifft_N(H)) and a[m] = (1/N) sum_h |Re(H_h w^(h m))|, w = exp(2 pi i / N) (the reference's hull), or
 * a = |g| (the exact interval hull of the same linear map).  The two tables are fp64 device arrays of N entries, built by the
 * caller; this library only applies them.
 *
 * Operands.  A row operand is B rows of N (or Nt) values, element (b, j) at ptr[b*s[0] + j*s[1]] (int64 element strides, any
 * sign; a zero stride broadcasts).  Outputs are dense fp64 [B, N] (row b at out + b*N) and must not alias an input.
 *
 * Arithmetic, fp64.  Each sum runs over j in ascending order with the same grouping on every call, so repeated calls give the
 * same bits.  Every output sums every input, so a NaN or inf anywhere in a row makes every bound of that row NaN (so does a
 * centre or radius that overflows); other rows are unaffected.
 *
 * Every call is asynchronous on the given HIP stream (NULL: the default stream), allocates nothing and never synchronises,
 * so a sequence of calls can be captured in a graph.  Return codes: 0 ok; < 0 PRE_E_* as in cp_pre_hip.h
 * (PRE_E_NULL: a null pointer or a negative size, PRE_E_SHAPE: N < 1, or Nt < 3 for the recipe, PRE_E_UNSUPPORTED: a kernel
 * of more than PRE_SETPROP_MAX_TAPS taps or more taps than Nt + 2, or q-hat given with a kernel whose index mapping is not
 * derived (below)); > 0 a hipError_t.
 */
#ifndef CP_PRE_SETPROP_H
#define CP_PRE_SETPROP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_SETPROP_ABI_VERSION 1
#define PRE_SETPROP_MAX_TAPS 7
#define PRE_SETPROP_FLAG_F64 1           /* bounds: centre and radius rows are double (else float) */
#define PRE_SETPROP_FLAG_CORRELATION 2   /* recipe: the kernel spectrum is conjugated (SHO.py set_PRE(correlation=True)) */

int pre_setprop_abi_version(void);

/* The general circulant hull: lower/upper[b, k] from the sets (centre[b, j] -+ radius[b, j]), j, k < N, with the tables g and
 * a (device, N doubles each).  radius must be >= 0 (not checked here). */
int pre_setprop_bounds_f64(const void *centre, const int64_t c_strides[2], const void *radius, const int64_t r_strides[2],
                           int64_t B, int64_t N, const double *g, const double *a, double *lower, double *upper, int flags,
                           void *stream);

/* The reference recipe, fused (SHO.py:360-407).  Field row b (Nt fp32 steps) is padded as s = [0, field, 0] (length Nt + 2),
 * convolved circularly with the k taps (host array, fp64) in fp64:
 *     conv[n] = sum_i taps[i] * s[(n - i) mod (Nt + 2)]          (flags without PRE_SETPROP_FLAG_CORRELATION)
 *     conv[n] = sum_i taps[i] * s[(n + i) mod (Nt + 2)]          (with it: the conjugated spectrum)
 * and turned into N = Nt + 1 intervals, j = n - 1: points conv[1..3] and conv[Nt + 1], symmetric [-|conv[n]|, |conv[n]|] for
 * n = 4 .. Nt.  g and a (N doubles each) are the tables of the reference's spectrum truncated to N entries.  Outputs are
 * lower/upper [B, Nt + 1].
 * qhat (NULL: none) replaces the interior radii |conv[n]| with conformal q-hat values (fp32, element (b, t) at
 * qhat[b*q_strides[0] + t*q_strides[1]], t < Nt: a scalar, a [Nt] row or [B, Nt]).  conv[n] is the residual (the
 * cross-correlation of Utils/ConvOps_0d.py, padding k/2) at step t = n - (k+1)/2 for a symmetric kernel without correlation,
 * and at t = n + (k-3)/2 for any kernel with it; k must be odd, and symmetric without correlation (else PRE_E_UNSUPPORTED).
 * An interior n whose step t falls outside [0, Nt) keeps |conv[n]|.  A non-finite field value makes its row NaN even where
 * q-hat replaces the radii it reaches. */
int pre_setprop_recipe_f32(const float *field, const int64_t f_strides[2], int64_t B, int64_t Nt, const double *taps, int k,
                           const float *qhat, const int64_t q_strides[2], const double *g, const double *a, double *lower,
                           double *upper, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif
