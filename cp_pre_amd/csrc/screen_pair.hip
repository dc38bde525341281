// screen_pair.hip - the calibrated-set screens of screen_march.hip (Ny-fastest fields) and screen_flat.hip (Nt-fastest
// fields) for the data-driven scores d = r(a) - r(b) of two field sets (libcp_pre_screenpair.so,
// include/cp_pre_screenpair.h): per sample, max |d| / m and the number of cells with |d| <= q_k * m at up to 16 levels, in
// the launch that evaluates both residuals.  Neither residual nor their difference is written.
//
// Nothing new runs on the device: the marches are screen_march.h's and screen_flat.h's, the functor is Paired<Fn>
// (paired_functor.h, shared with pair_march.hip) over star_march.h's Linear1, Linear2, NSMomentum and MHDContinuity - views
// [0, F) the truth set, [F, 2F) the prediction set, each half rounded to fp32 before the subtraction.  The host side of an
// entry is screen_entries.h's: the entry hands the 2F views of both sets (pair_views) to the body of its kind with <Form, Paired,
// ScalarSets>, so every check of host_checks.h is made of every view of both sets; this object's flags are star_march.o's
// (csrc/Makefile), so each half in registers is the residual the single-set pass would have stored.
//
// Built: Paired<Linear1>, Paired<Linear2>, and Paired<NSMomentum<M>> / Paired<MHDContinuity<M>> in the reference's tap
// structure and the y-fixed one (M = 0, 1 Ny-fastest; 3, 4 Nt-fastest) - but for Paired<NSMomentum<4>>; their general stars
// are not built either (the table Built of screen_entries.h, with the figures).  The entry returns PRE_E_UNSUPPORTED for a
// tap structure that is not built.  No instantiation that is built has scratch (resources.sh screen_pair.hip).
#include "screen_march.h"
#include "screen_flat.h"
#include "paired_functor.h"
#include "../../include/cp_pre_screenpair.h"
#include "screen_entries.h"

extern "C" {

int pre_screenpair_abi_version(void) { return PRE_SCREENPAIR_ABI_VERSION; }

// ---------------------------------------------------------------- Ny-fastest fields: screen_march.h
int pre_screenpair_stencil3d_f32(const pre_field_t *a, const pre_field_t *b, const float *tap_w, const int32_t *tap_off, int ntaps,
                                 const pre_screen_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return stencil3d<NyForm, Paired, ScalarSets>({{a, b}, 2}, tap_w, tap_off, ntaps, s, B, T, X, Y, flags, stream);
}

int pre_screenpair_linear2_f32(const pre_field_t a[2], const pre_field_t b[2], const float *K_a, const float *K_b, float ratio,
                               const pre_screen_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!a || !b) return PRE_E_NULL;
    return linear2<NyForm, Paired, ScalarSets>(pair_views<2>(a, b), K_a, K_b, ratio, s, B, T, X, Y, flags, stream);
}

int pre_screenpair_ns_momentum_f32(const pre_field_t a[3], const pre_field_t b[3], const float *K_t, const float *K_x,
                                   const float *K_y, const float *K_xx_yy, float dt, float dx, float dy, float nu,
                                   const pre_screen_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!a || !b) return PRE_E_NULL;
    return ns_momentum<NyForm, Paired, ScalarSets>(pair_views<3>(a, b), K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu, s, B, T, X, Y,
                                                   flags, stream);
}

int pre_screenpair_mhd_continuity_f32(const pre_field_t a[3], const pre_field_t b[3], const float *K_t, const float *K_x,
                                      const float *K_y, double gamma, const pre_screen_t *s, int64_t B, int64_t T, int64_t X,
                                      int64_t Y, int flags, void *stream)
{
    if (!a || !b) return PRE_E_NULL;
    return mhd<NyForm, Paired, ScalarSets>(0, pair_views<3>(a, b), K_t, K_x, K_y, gamma, s, B, T, X, Y, flags, stream);
}

// ---------------------------------------------------------------- Nt-fastest fields: screen_flat.h
int pre_screenpair_flat_stencil3d_f32(const pre_field_t *a, const pre_field_t *b, const float *tap_w, const int32_t *tap_off,
                                      int ntaps, const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                      void *stream)
{
    return stencil3d<FlatForm, Paired, ScalarSets>({{a, b}, 2}, tap_w, tap_off, ntaps, s, B, T, X, Y, flags, stream);
}

int pre_screenpair_flat_linear2_f32(const pre_field_t a[2], const pre_field_t b[2], const float *K_a, const float *K_b,
                                    float ratio, const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                    void *stream)
{
    if (!a || !b) return PRE_E_NULL;
    return linear2<FlatForm, Paired, ScalarSets>(pair_views<2>(a, b), K_a, K_b, ratio, s, B, T, X, Y, flags, stream);
}

int pre_screenpair_flat_ns_momentum_f32(const pre_field_t a[3], const pre_field_t b[3], const float *K_t, const float *K_x,
                                        const float *K_y, const float *K_xx_yy, float dt, float dx, float dy, float nu,
                                        const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                        void *stream)
{
    if (!a || !b) return PRE_E_NULL;
    return ns_momentum<FlatForm, Paired, ScalarSets>(pair_views<3>(a, b), K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu, s, B, T, X, Y,
                                                     flags, stream);
}

int pre_screenpair_flat_mhd_continuity_f32(const pre_field_t a[3], const pre_field_t b[3], const float *K_t, const float *K_x,
                                           const float *K_y, double gamma, const pre_screenflat_t *s, int64_t B, int64_t T,
                                           int64_t X, int64_t Y, int flags, void *stream)
{
    if (!a || !b) return PRE_E_NULL;
    return mhd<FlatForm, Paired, ScalarSets>(0, pair_views<3>(a, b), K_t, K_x, K_y, gamma, s, B, T, X, Y, flags, stream);
}

}  // extern "C"
