// screen_pair.hip - the calibrated-set screens of screen_march.hip (Ny-fastest fields) and screen_flat.hip (Nt-fastest
// fields) for the data-driven scores d = r(a) - r(b) of two field sets (libcp_pre_screenpair.so,
// include/cp_pre_screenpair.h): per sample, max |d| / m and the number of cells with |d| <= q_k * m at up to 16 levels, in
// the launch that evaluates both residuals.  Neither residual nor their difference is written.
//
// Nothing new runs on the device: the marches are screen_march.h's and screen_flat.h's, the functor is Paired<Fn>
// (paired_functor.h, shared with pair_march.hip) over star_march.h's Linear1, Linear2, NSMomentum and MHDContinuity - views
// [0, F) the truth set, [F, 2F) the prediction set, each half rounded to fp32 before the subtraction.  The host side of an
// entry is its single-set twin's (screen_march.hip, screen_flat.hip) with 2F views handed to prepare_screen / prepare_flat,
// so every check of host_checks.h is made of every view of both sets; this object's flags are star_march.o's (csrc/Makefile),
// so each half in registers is the residual the single-set pass would have stored.
//
// Built: Paired<Linear1>, Paired<Linear2>, and Paired<NSMomentum<M>> / Paired<MHDContinuity<M>> in the reference's tap
// structure and the y-fixed one (M = 0, 1 Ny-fastest; 3, 4 Nt-fastest) - but for Paired<NSMomentum<4>>, which would carry 8
// bytes of scratch.  Their general stars are not built either, as in libcp_pre_pair.so.  The entry returns
// PRE_E_UNSUPPORTED for a tap structure that is not built.  No instantiation that is built has scratch (resources.sh
// screen_pair.hip).
#include "screen_march.h"
#include "screen_flat.h"
#include "paired_functor.h"
#include "../../include/cp_pre_screenpair.h"

namespace {

// The tap structures built for the six-view paired functors; mode on the kernel's axes (relabeled_mode for the flat form).
// On the 512-thread tiles of launch_screen the paired NS momentum takes 250-256 registers and the paired MHD continuity
// 169-199, none with scratch, so the tiles stay launch_screen's.
template <template <int> class FnT, class P>
int launch_pair6_mode(int mode, SGeom &g, const P &prm, hipStream_t st)
{
    if (mode == 0) return launch_screen<FnT<0>>(g, prm, st);
    if (mode == 1) return launch_screen<FnT<1>>(g, prm, st);
    return PRE_E_UNSUPPORTED;
}

// YFIXED: is the y-fixed tap structure (<4>) built?  Paired<NSMomentum<4>> stages all six fields in the merged-row march and
// does not fit the 256 registers of its 512-thread chunk with the epilogue (8 bytes of scratch): not built, as
// MHDMomentum<2> in libcp_pre_screenflat.so; the caller takes its three-pass route.
template <template <int> class FnT, bool YFIXED, class P>
int launch_pair6_flat_mode(int mode, FGeom &g, const P &prm, hipStream_t st)
{
    if (mode == 3) return launch_screen_flat<FnT<3>>(g, prm, st);
    if constexpr (YFIXED)
        if (mode == 4) return launch_screen_flat<FnT<4>>(g, prm, st);
    return PRE_E_UNSUPPORTED;
}

int ns_params(NSParams &prm, int *mode, const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy, float dt,
              float dx, float dy, float nu)
{
    if (!star_from_dense27(K_t, &prm.Dt) || !star_from_dense27(K_x, &prm.Dx) || !star_from_dense27(K_y, &prm.Dy) ||
        !star_from_dense27(K_xx_yy, &prm.L))
        return PRE_E_UNSUPPORTED;
    *mode = pick_mode(prm.Dt, prm.Dx, prm.Dy, &prm.L);      // on the caller's axes
    prm.dxdy = dx * dy; prm.dtdy = dt * dy; prm.dtdx = dt * dx; prm.nudt = nu * dt;      // (as pre_residual_ns_momentum_f32)
    return PRE_OK;
}

int mhd_params(MHDParams &prm, int *mode, const float *K_t, const float *K_x, const float *K_y, double gamma)
{
    if (!star_from_dense27(K_t, &prm.Dt) || !star_from_dense27(K_x, &prm.Dx) || !star_from_dense27(K_y, &prm.Dy))
        return PRE_E_UNSUPPORTED;
    prm.gamma = (float)gamma;
    prm.gm2 = (float)(gamma - 2.0);   // (as pre_residual_mhd_f32)
    *mode = pick_mode(prm.Dt, prm.Dx, prm.Dy, nullptr);
    return PRE_OK;
}

}  // namespace

extern "C" {

int pre_screenpair_abi_version(void) { return PRE_SCREENPAIR_ABI_VERSION; }

// ---------------------------------------------------------------- Ny-fastest fields: screen_march.h
int pre_screenpair_stencil3d_f32(const pre_field_t *a, const pre_field_t *b, const float *tap_w, const int32_t *tap_off, int ntaps,
                                 const pre_screen_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    const pre_field_t *fs[2] = {a, b};
    SGeom g;
    int rc = prepare_screen(g, fs, 2, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear1::Params p;
    if (!star_of_taps(tap_w, tap_off, ntaps, &p.s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    Star *stars[1] = {&p.s};
    g.tfree = no_t_taps(stars, 1);
    return launch_screen<Paired<Linear1>>(g, p, as_stream(stream));
}

int pre_screenpair_linear2_f32(const pre_field_t a[2], const pre_field_t b[2], const float *K_a, const float *K_b, float ratio,
                               const pre_screen_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!a || !b || !K_a || !K_b) return PRE_E_NULL;
    const pre_field_t *fs[4] = {&a[0], &a[1], &b[0], &b[1]};
    SGeom g;
    int rc = prepare_screen(g, fs, 4, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear2::Params prm;
    if (!star_from_dense27(K_a, &prm.a) || !star_from_dense27(K_b, &prm.b)) return PRE_E_UNSUPPORTED;
    prm.ratio = ratio;
    Star *stars[2] = {&prm.a, &prm.b};
    g.tfree = no_t_taps(stars, 2);
    return launch_screen<Paired<Linear2>>(g, prm, as_stream(stream));
}

int pre_screenpair_ns_momentum_f32(const pre_field_t a[3], const pre_field_t b[3], const float *K_t, const float *K_x,
                                   const float *K_y, const float *K_xx_yy, float dt, float dx, float dy, float nu,
                                   const pre_screen_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!a || !b || !K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    const pre_field_t *fs[6] = {&a[0], &a[1], &a[2], &b[0], &b[1], &b[2]};
    SGeom g;
    int rc = prepare_screen(g, fs, 6, s, B, T, X, Y, flags);
    if (rc) return rc;
    NSParams prm;
    int mode;
    rc = ns_params(prm, &mode, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu);
    if (rc) return rc;
    Star *stars[4] = {&prm.Dt, &prm.Dx, &prm.Dy, &prm.L};
    g.tfree = no_t_taps(stars, 4);
    return launch_pair6_mode<PairedNS>(mode, g, prm, as_stream(stream));
}

int pre_screenpair_mhd_continuity_f32(const pre_field_t a[3], const pre_field_t b[3], const float *K_t, const float *K_x,
                                      const float *K_y, double gamma, const pre_screen_t *s, int64_t B, int64_t T, int64_t X,
                                      int64_t Y, int flags, void *stream)
{
    if (!a || !b || !K_t || !K_x || !K_y) return PRE_E_NULL;
    const pre_field_t *fs[6] = {&a[0], &a[1], &a[2], &b[0], &b[1], &b[2]};
    SGeom g;
    int rc = prepare_screen(g, fs, 6, s, B, T, X, Y, flags);
    if (rc) return rc;
    MHDParams prm;
    int mode;
    rc = mhd_params(prm, &mode, K_t, K_x, K_y, gamma);
    if (rc) return rc;
    Star *stars[3] = {&prm.Dt, &prm.Dx, &prm.Dy};
    g.tfree = no_t_taps(stars, 3);
    return launch_pair6_mode<PairedMHDContinuity>(mode, g, prm, as_stream(stream));
}

// ---------------------------------------------------------------- Nt-fastest fields: screen_flat.h
int pre_screenpair_flat_stencil3d_f32(const pre_field_t *a, const pre_field_t *b, const float *tap_w, const int32_t *tap_off,
                                      int ntaps, const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                      void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    const pre_field_t *fs[2] = {a, b};
    FGeom g;
    int rc = prepare_flat(g, fs, 2, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear1::Params p;
    if (!star_of_taps(tap_w, tap_off, ntaps, &p.s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    Star *stars[1] = {&p.s};
    relabel_stars(stars, 1);
    return launch_screen_flat<Paired<Linear1>>(g, p, as_stream(stream));
}

int pre_screenpair_flat_linear2_f32(const pre_field_t a[2], const pre_field_t b[2], const float *K_a, const float *K_b,
                                    float ratio, const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                    void *stream)
{
    if (!a || !b || !K_a || !K_b) return PRE_E_NULL;
    const pre_field_t *fs[4] = {&a[0], &a[1], &b[0], &b[1]};
    FGeom g;
    int rc = prepare_flat(g, fs, 4, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear2::Params prm;
    if (!star_from_dense27(K_a, &prm.a) || !star_from_dense27(K_b, &prm.b)) return PRE_E_UNSUPPORTED;
    prm.ratio = ratio;
    Star *stars[2] = {&prm.a, &prm.b};
    relabel_stars(stars, 2);
    return launch_screen_flat<Paired<Linear2>>(g, prm, as_stream(stream));
}

int pre_screenpair_flat_ns_momentum_f32(const pre_field_t a[3], const pre_field_t b[3], const float *K_t, const float *K_x,
                                        const float *K_y, const float *K_xx_yy, float dt, float dx, float dy, float nu,
                                        const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                        void *stream)
{
    if (!a || !b || !K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    const pre_field_t *fs[6] = {&a[0], &a[1], &a[2], &b[0], &b[1], &b[2]};
    FGeom g;
    int rc = prepare_flat(g, fs, 6, s, B, T, X, Y, flags);
    if (rc) return rc;
    NSParams prm;
    int mode;
    rc = ns_params(prm, &mode, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu);
    if (rc) return rc;
    Star *stars[4] = {&prm.Dt, &prm.Dx, &prm.Dy, &prm.L};
    relabel_stars(stars, 4);
    return launch_pair6_flat_mode<PairedNS, false>(relabeled_mode(mode, 1), g, prm, as_stream(stream));
}

int pre_screenpair_flat_mhd_continuity_f32(const pre_field_t a[3], const pre_field_t b[3], const float *K_t, const float *K_x,
                                           const float *K_y, double gamma, const pre_screenflat_t *s, int64_t B, int64_t T,
                                           int64_t X, int64_t Y, int flags, void *stream)
{
    if (!a || !b || !K_t || !K_x || !K_y) return PRE_E_NULL;
    const pre_field_t *fs[6] = {&a[0], &a[1], &a[2], &b[0], &b[1], &b[2]};
    FGeom g;
    int rc = prepare_flat(g, fs, 6, s, B, T, X, Y, flags);
    if (rc) return rc;
    MHDParams prm;
    int mode;
    rc = mhd_params(prm, &mode, K_t, K_x, K_y, gamma);
    if (rc) return rc;
    Star *stars[3] = {&prm.Dt, &prm.Dx, &prm.Dy};
    relabel_stars(stars, 3);
    return launch_pair6_flat_mode<PairedMHDContinuity, true>(relabeled_mode(mode, 1), g, prm, as_stream(stream));
}

}  // extern "C"
