// vjp_mhd.hip - vector-Jacobian products of the ideal-MHD residuals (libcp_pre_vjpmhd.so, include/cp_pre_vjpmhd.h): the
// backward pass of a physics-informed loss on MHD.residual_{continuity,induction,momentum,energy}.
//
// The march is vjp_march.h's (shared with residual_vjp.hip), the functors are vjp_functors.h's.  Continuity and induction
// are one launch each; momentum and energy are two launches each, split by output group: in one pass (7 / 6 streams in, 6
// out) they need scratch in every tap structure.  The functors are templated on the MODE of the forward march (0: the
// reference's construction - D_t and D_y along Nt, D_x along Nx; 1: D_y along Ny; 2: general stars); a MODE whose
// instantiation needs scratch is not built and its entry returns PRE_E_UNSUPPORTED before any launch (VJPMHD_MODE2_*
// below; the table: DESIGN 4.19, re-measure with resources.sh when a functor or the march changes).
#include "vjp_march.h"
#include "../../include/cp_pre_vjpmhd.h"

// is the general-star instantiation of an equation built?  (momentum: both passes)
#ifndef VJPMHD_MODE2_CONTINUITY
#define VJPMHD_MODE2_CONTINUITY 0
#endif
#ifndef VJPMHD_MODE2_INDUCTION
#define VJPMHD_MODE2_INDUCTION 0
#endif
#ifndef VJPMHD_MODE2_MOMENTUM
#define VJPMHD_MODE2_MOMENTUM 1
#endif
#ifndef VJPMHD_MODE2_ENERGY
#define VJPMHD_MODE2_ENERGY 0
#endif

namespace {

constexpr bool MODE2_BUILT[4] = {VJPMHD_MODE2_CONTINUITY != 0, VJPMHD_MODE2_MOMENTUM != 0, VJPMHD_MODE2_ENERGY != 0,
                                 VJPMHD_MODE2_INDUCTION != 0};          // by PRE_VJPMHD_EQ_*

struct Stars { Star Dt, Dx, Dy; int mode; };

// the three operators of an equation and the tap structure they fit; PRE_E_UNSUPPORTED for weight off the star or for a
// structure whose instantiation is not built
int stars_of(int eq, const float *K_t, const float *K_x, const float *K_y, Stars *s)
{
    if (!K_t || !K_x || !K_y) return PRE_E_NULL;
    if (!star_from_dense27(K_t, &s->Dt) || !star_from_dense27(K_x, &s->Dx) || !star_from_dense27(K_y, &s->Dy))
        return PRE_E_UNSUPPORTED;
    s->mode = pick_mode(s->Dt, s->Dx, s->Dy, nullptr);
    return (s->mode == 2 && !MODE2_BUILT[eq]) ? PRE_E_UNSUPPORTED : PRE_OK;
}

const Star ZERO{0, 0, 0, 0, 0, 0, 0};
Star plus(const Star &a, const Star &b) { return combine(1.0, a, 1.0, b); }
Star minus(const Star &a, const Star &b) { return combine(1.0, a, -1.0, b); }
Star twice(const Star &a) { return combine(2.0, a, 0.0, ZERO); }

VjpMHDStars plain_stars(const Stars &s) { return VjpMHDStars{mirrored(s.Dt), s.Dx, s.Dy, mirrored(s.Dx), mirrored(s.Dy)}; }

// the geometry of one launch: streams `in` (0 is g) and outputs `out` of the checked geometry of all of them
VGeom pass_of(const VGeom &all, const int *in, int nin, const int *out, int nout)
{
    VGeom g = all;
    for (int i = 0; i < VJP_MAXIN; ++i) {
        const bool on = i < nin;
        g.f[i] = on ? all.f[in[i]] : nullptr;
        g.sB[i] = on ? all.sB[in[i]] : 0; g.sT[i] = on ? all.sT[in[i]] : 0; g.sX[i] = on ? all.sX[in[i]] : 0;
    }
    for (int k = 0; k < VJP_MAXOUT; ++k) {
        const bool on = k < nout;
        g.o[k] = on ? all.o[out[k]] : nullptr;
        g.oB[k] = on ? all.oB[out[k]] : 0; g.oT[k] = on ? all.oT[out[k]] : 0; g.oX[k] = on ? all.oX[out[k]] : 0;
    }
    return g;
}

template <template <int> class Fn, bool MODE2>
int launch_mode(int mode, VGeom &g, const typename Fn<0>::Params &p, hipStream_t st)
{
    static_assert(std::is_same<typename Fn<0>::Params, typename Fn<1>::Params>::value &&
                  std::is_same<typename Fn<0>::Params, typename Fn<2>::Params>::value, "one Params for every MODE");
    if (mode == 0) return launch_vjp<Fn<0>>(g, p, st);
    if (mode == 1) return launch_vjp<Fn<1>>(g, p, st);
    if constexpr (MODE2) return launch_vjp<Fn<2>>(g, p, st);
    return PRE_E_UNSUPPORTED;                            // (not reached: stars_of has declined)
}

// g and the nf fields in, the nf gradients out: every view checked once, all of them against each other
int prepare_all(VGeom &vg, const pre_field_t *g, const pre_field_t *fields, const pre_out_t *out, int nf, int64_t B, int64_t T,
                int64_t X, int64_t Y, int flags, float host_scale, const float *dev_scale)
{
    const pre_field_t *fs[VJP_MAXIN] = {g};
    const pre_out_t *os[VJP_MAXOUT] = {};
    for (int i = 0; i < nf; ++i) { fs[1 + i] = &fields[i]; os[i] = &out[i]; }
    return prepare_vjp(vg, fs, 1 + nf, os, nf, B, T, X, Y, crop_of(flags, false), host_scale, dev_scale);
}

}  // namespace

extern "C" {

int pre_vjpmhd_abi_version(void) { return PRE_VJPMHD_ABI_VERSION; }

int pre_vjpmhd_supported(int eq, const float *K_t, const float *K_x, const float *K_y)
{
    if (eq < 0 || eq > 3) return PRE_E_RANGE;
    Stars s;
    return stars_of(eq, K_t, K_x, K_y, &s);
}

int pre_vjpmhd_continuity_f32(const pre_field_t *g, const pre_field_t fields[3], const pre_out_t out[3], const float *K_t,
                              const float *K_x, const float *K_y, float host_scale, const float *dev_scale, int64_t B,
                              int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !out || !K_t || !K_x || !K_y) return PRE_E_NULL;
    VGeom vg;
    Stars s;
    int rc = prepare_all(vg, g, fields, out, 3, B, T, X, Y, flags, host_scale, dev_scale);
    if (rc) return rc;
    if ((rc = stars_of(PRE_VJPMHD_EQ_CONTINUITY, K_t, K_x, K_y, &s))) return rc;
    vg.tfree = !has_t(s.Dt) && !has_t(s.Dx) && !has_t(s.Dy);
    return launch_mode<VjpMHDContinuity, VJPMHD_MODE2_CONTINUITY != 0>(s.mode, vg, plain_stars(s), as_stream(stream));
}

int pre_vjpmhd_induction_f32(const pre_field_t *g, const pre_field_t fields[4], const pre_out_t out[4], const float *K_t,
                             const float *K_x, const float *K_y, float host_scale, const float *dev_scale, int64_t B,
                             int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !out || !K_t || !K_x || !K_y) return PRE_E_NULL;
    VGeom vg;
    Stars s;
    int rc = prepare_all(vg, g, fields, out, 4, B, T, X, Y, flags, host_scale, dev_scale);
    if (rc) return rc;
    if ((rc = stars_of(PRE_VJPMHD_EQ_INDUCTION, K_t, K_x, K_y, &s))) return rc;
    vg.tfree = !has_t(s.Dt) && !has_t(s.Dx) && !has_t(s.Dy);
    const Star M = minus(s.Dx, s.Dy), P = plus(s.Dx, s.Dy);
    const VjpMHDInductionParams p{mirrored(s.Dt), M, P, mirrored(M), mirrored(P)};
    return launch_mode<VjpMHDInduction, VJPMHD_MODE2_INDUCTION != 0>(s.mode, vg, p, as_stream(stream));
}

int pre_vjpmhd_momentum_f32(const pre_field_t *g, const pre_field_t fields[6], const pre_out_t out[6], const float *K_t,
                            const float *K_x, const float *K_y, float host_scale, const float *dev_scale, int64_t B,
                            int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !out || !K_t || !K_x || !K_y) return PRE_E_NULL;
    VGeom vg;
    Stars s;
    int rc = prepare_all(vg, g, fields, out, 6, B, T, X, Y, flags, host_scale, dev_scale);
    if (rc) return rc;
    if ((rc = stars_of(PRE_VJPMHD_EQ_MOMENTUM, K_t, K_x, K_y, &s))) return rc;
    vg.tfree = !has_t(s.Dt) && !has_t(s.Dx) && !has_t(s.Dy);
    // streams of the checked geometry: 0 g, 1 rho, 2 u, 3 v, 4 p, 5 Bx, 6 By; outputs in the order of the fields
    const int inA[3] = {0, 2, 3}, outA[2] = {1, 2}, inB[5] = {0, 1, 4, 5, 6}, outB[4] = {0, 3, 4, 5};
    VGeom a = pass_of(vg, inA, 3, outA, 2), b = pass_of(vg, inB, 5, outB, 4);
    const Star P = plus(s.Dx, s.Dy), D2x = twice(s.Dx), D2y = twice(s.Dy);
    const VjpMHDMomentumBParams pb{P, mirrored(P), D2x, D2y, mirrored(D2x), mirrored(D2y)};
    hipStream_t st = as_stream(stream);
    if ((rc = launch_mode<VjpMHDMomentumA, VJPMHD_MODE2_MOMENTUM != 0>(s.mode, a, plain_stars(s), st))) return rc;
    return launch_mode<VjpMHDMomentumB, VJPMHD_MODE2_MOMENTUM != 0>(s.mode, b, pb, st);
}

int pre_vjpmhd_energy_f32(const pre_field_t *g, const pre_field_t fields[6], const pre_out_t out[6], const float *K_t,
                          const float *K_x, const float *K_y, double gamma, float host_scale, const float *dev_scale,
                          int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !out || !K_t || !K_x || !K_y) return PRE_E_NULL;
    VGeom vg;
    Stars s;
    int rc = prepare_all(vg, g, fields, out, 6, B, T, X, Y, flags, host_scale, dev_scale);
    if (rc) return rc;
    if ((rc = stars_of(PRE_VJPMHD_EQ_ENERGY, K_t, K_x, K_y, &s))) return rc;
    vg.tfree = !has_t(s.Dt) && !has_t(s.Dx) && !has_t(s.Dy);
    const int inA[4] = {0, 4, 5, 6}, outA[3] = {0, 1, 2}, inB[5] = {0, 2, 3, 5, 6}, outB[3] = {3, 4, 5};
    VGeom a = pass_of(vg, inA, 4, outA, 3), b = pass_of(vg, inB, 5, outB, 3);
    const VjpMHDStars ps = plain_stars(s);
    // "(gamma-2)" is a float64 Python scalar in the reference: rounded once, as pre_residual_mhd_f32 does
    const VjpMHDEnergyParams p{ps.DtT, ps.Dx, ps.Dy, ps.DxT, ps.DyT, (float)gamma, (float)(gamma - 2.0)};
    hipStream_t st = as_stream(stream);
    if ((rc = launch_mode<VjpMHDEnergyA, VJPMHD_MODE2_ENERGY != 0>(s.mode, a, p, st))) return rc;
    return launch_mode<VjpMHDEnergyB, VJPMHD_MODE2_ENERGY != 0>(s.mode, b, p, st);
}

}  // extern "C"
