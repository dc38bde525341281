// screen_rows_pair.hip - the calibrated-set screen of screen_rows.hip for the data-driven scores d = r(a) - r(b) of two
// [B,Nt,Nx] field sets (libcp_pre_screen1dpair.so, include/cp_pre_screen1dpair.h): per sample, max |d| / m and the number
// of cells with |d| <= q_k * m at up to 16 levels, in the launch that evaluates both residuals.  Neither residual nor their
// difference is written.
//
// The march is screen_rows.h's - stated once, for one or two field sets - with the functor Paired<Fn> (paired_functor.h,
// shared with pair_march.hip and screen_pair.hip) over star_march.h's Linear1 and Burgers<MODE>: view 0 the truth set, view 1
// the prediction set, each half rounded to fp32 before the subtraction.  Per wave: rows r-1, r, r+1 of its own quads of BOTH
// sets in registers, row r+2 of both in flight, one edge scalar per set, the modulation as one float4 stream; no LDS and no
// barrier inside the march; the split, the end of a row, the combine step and the atomics are the single-set screen's.  Each
// set has its own sample and row pitch; both must have their unit stride on the same axis (prepare_rows).
//
// Semantics: the one-sided test |d| <= q_k * m on the difference - what pre_pair_*_f32, the joint score and
// pre_cov_levels_f32 give in three passes - NOT the reference's two-sided form c - hw <= y <= c + hw on the two residual
// arrays.
//
// The file is compiled twice (Makefile), as pair_march.hip is.  PRE_SCREEN1DPAIR_PART 1, with star_march.o's flags: the
// tap-list entry (Paired<Linear1>) and the version.  PRE_SCREEN1DPAIR_PART 2, without fma contraction: the Burgers entry -
// contracted, the compiler may fuse the two halves of Paired<Burgers> differently and minus == vars then gives 1-ulp
// differences instead of 0.  hw = q_k * m is uncontracted in both (screen_plane.h).  No instantiation has
// scratch (resources.sh screen_rows_pair.hip with HIPCC_EXTRA of the part).
#ifndef PRE_SCREEN1DPAIR_PART
#error "PRE_SCREEN1DPAIR_PART: 1 or 2 (see the Makefile)"
#endif
#include "screen_rows.h"
#include "paired_functor.h"
#include "../../include/cp_pre_screen1dpair.h"

extern "C" {

#if PRE_SCREEN1DPAIR_PART == 1

int pre_screen1dpair_abi_version(void) { return PRE_SCREEN1DPAIR_ABI_VERSION; }

int pre_screen1dpair_stencil2d_f32(const float *a, const int64_t strides_a[3], const float *b, const int64_t strides_b[3],
                                   const float *tap_w, const int32_t *tap_off, int ntaps, const pre_screen_t *s, int64_t B,
                                   int64_t T, int64_t X, int flags, void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 49) return PRE_E_SHAPE;
    const float *u[2] = {a, b};
    const int64_t *st[2] = {strides_a, strides_b};
    RGeom g;
    int nt_fast = 0;
    int rc = prepare_rows(g, &nt_fast, u, st, 2, s, B, T, X, flags);
    if (rc) return rc;
    float k9[9];
    bool star;
    rc = rows_dense9_of_taps(tap_w, tap_off, ntaps, k9, &star);
    if (rc) return rc;
    if (!star) return PRE_E_UNSUPPORTED;
    Linear1::Params p;
    rows_star_from_dense9(k9, nt_fast, &p.s);
    return launch_rows<Paired<Linear1>>(g, p, as_stream(stream));
}

#endif  // PRE_SCREEN1DPAIR_PART == 1
#if PRE_SCREEN1DPAIR_PART == 2

int pre_screen1dpair_burgers_f32(const float *a, const int64_t strides_a[3], const float *b, const int64_t strides_b[3],
                                 const float *K_t, const float *K_x, const float *K_xx, float dx, float dt, float nu, float c3,
                                 const pre_screen_t *s, int64_t B, int64_t T, int64_t X, int flags, void *stream)
{
    if (!K_t || !K_x || !K_xx) return PRE_E_NULL;
    const float *u[2] = {a, b};
    const int64_t *st[2] = {strides_a, strides_b};
    RGeom g;
    int nt_fast = 0, mode;
    int rc = prepare_rows(g, &nt_fast, u, st, 2, s, B, T, X, flags);
    if (rc) return rc;
    BurgersParams prm;
    rc = rows_burgers_params(prm, &mode, nt_fast, K_t, K_x, K_xx, dx, dt, nu, c3);
    if (rc) return rc;
    hipStream_t hs = as_stream(stream);
    if (mode == 0) return launch_rows<Paired<Burgers<0>>>(g, prm, hs);
    if (mode == 3) return launch_rows<Paired<Burgers<3>>>(g, prm, hs);
    return launch_rows<Paired<Burgers<2>>>(g, prm, hs);
}

#endif  // PRE_SCREEN1DPAIR_PART == 2

}  // extern "C"
