/* cp_pre_ode.h - C ABI of libcp_pre_ode.so: the ODE operators of the reference's Utils/ConvOps_0d.py (a [BS, Nt] field
 * cross-correlated with a 3-, 5- or 7-tap stencil, F.conv1d(x[:, None], K[None, None], padding=k//2)) and the fused ODE
 * residuals built from them (Inverse_residuals/SHO/SHO_node_test.py:341-345, Inverse_residuals/DHO/DHO_NODE.py:475-483,
 * 509-513, 559-563, Inverse_residuals/Bessel/Bessel_NODE.py:493-518).  Served by cp_pre_amd.convops_0d and cp_pre_amd.ode.
 *
 * Operands.  A field is BS rows of Nt steps, element (b, t) at ptr[b*s[0] + t*s[1]] (int64 element strides, any sign;
 * a zero batch stride broadcasts one row).  So a component view sol[..., c] of a [BS, Nt, S] state tensor, a transposed
 * [Nt, BS] buffer or a row-padded score buffer is read or written where it lies.  An output must not overlap itself
 * (PRE_E_SHAPE: a zero stride on an axis longer than 1, or rows that interleave) and must not alias an input.
 *
 * Arithmetic, fp32: for each term, (K ⋆ x)[b, t] = sum_{j < k} taps[j] * x[b, t + j - k/2], the taps summed in order and
 * x taken as 0 outside [0, Nt).  Every tap of the term's window is multiplied, zero taps included, so a NaN or inf at t
 * reaches every output whose window covers t, as F.conv1d propagates it.
 *
 * Every call is asynchronous on the given HIP stream (NULL: the default stream), allocates nothing and never
 * synchronises, so a sequence of calls can be captured in a graph.  Return codes: 0 ok; < 0 PRE_E_* as in cp_pre_hip.h
 * (PRE_E_UNSUPPORTED: a kernel length that is even or above PRE_ODE_MAX_TAPS, or more than PRE_ODE_MAX_TERMS terms);
 * > 0 a hipError_t.
 */
#ifndef CP_PRE_ODE_H
#define CP_PRE_ODE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRE_ODE_ABI_VERSION 1
#define PRE_ODE_MAX_TAPS 7            /* k is odd, 1 <= k <= 7 */
#define PRE_ODE_MAX_TERMS 6
#define PRE_ODE_FLAG_ABS 1            /* store |out| (the marginal score) */
#define PRE_ODE_WGRAD_BLOCKS 1024     /* fp64 partials per tap of pre_ode_wgrad_f32: work holds this many * k doubles */

/* One term of a residual: c[t] * (K ⋆ x)[b, t].  x and c are device pointers, taps live in the struct (host). */
typedef struct {
    const float *x;           /* field, element (b, t) at x[b*sB + t*sT] */
    int64_t sB, sT;
    const float *c;           /* NULL (coefficient 1) or Nt per-step coefficients, dense */
    int k;                    /* odd, <= PRE_ODE_MAX_TAPS */
    float taps[PRE_ODE_MAX_TAPS];   /* taps[0 .. k-1] */
} pre_ode_term_t;

int pre_ode_abi_version(void);

/* out[b, t] = (K ⋆ in)[b, t]; `taps` is a host array of k floats. */
int pre_ode_stencil_f32(const float *in, const int64_t in_strides[2], float *out, const int64_t out_strides[2],
                        int64_t BS, int64_t Nt, const float *taps, int k, int flags, void *stream);

/* out[b, t] = sum_i c_i[t] * (K_i ⋆ x_i)[b, t] for 1 <= nterms <= PRE_ODE_MAX_TERMS (`terms` is a host array).  Terms that
 * name the same field view (x, sB, sT) share one load of it; the components of one [BS, Nt, S] tensor are loaded by the
 * same lanes in the same pass, so each of its cache lines is fetched once, not once per term. */
int pre_ode_residual_f32(const pre_ode_term_t *terms, int nterms, float *out, const int64_t out_strides[2],
                         int64_t BS, int64_t Nt, int flags, void *stream);

/* dk[j] = sum_{b, t} g[b, t] * x[b, t + j - k/2] (fp32 result): the kernel gradient of pre_ode_stencil_f32.  Deterministic:
 * PRE_ODE_WGRAD_BLOCKS workgroups each reduce a fixed range of (b, t) in fp64 into work[block * k + j] (device, at least
 * PRE_ODE_WGRAD_BLOCKS * k doubles), then one workgroup sums the partials in a fixed order.  No atomics. */
int pre_ode_wgrad_f32(const float *x, const int64_t x_strides[2], const float *g, const int64_t g_strides[2],
                      int64_t BS, int64_t Nt, int k, double *work, float *dk, void *stream);

#ifdef __cplusplus
}
#endif
#endif
