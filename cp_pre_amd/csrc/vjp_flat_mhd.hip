// vjp_flat_mhd.hip - the vector-Jacobian products of vjp_mhd.hip for Nt-fastest views of the ideal-MHD residuals
// (libcp_pre_vjpflatmhd.so, include/cp_pre_vjpflatmhd.h): the backward pass of a physics-informed loss on
// MHD.residual_{continuity,induction,momentum,energy}(pred.permute(0,1,4,2,3)), the view the reference's MHD callers pass.
//
// Nothing is marched here that is not marched elsewhere: the march, its geometry, its split and its layout checks are
// vjp_flat.hip's, included below without its entry points and with room for five input and four output streams (VF_MAXIN,
// VF_MAXOUT); the functors are vjp_functors.h's VjpMHD*<MODE>, instantiated for the tap structures the forward march has
// for this layout (star_march.h, relabeled_mode): 3 - the reference's construction seen on the kernel's axes (D_t and D_y
// along kernel y, D_x along the marched axis), 4 - y_axis_fix (D_y along kernel x), 2 - general stars.  The stars are
// mirrored and folded on the host in double exactly as vjp_mhd.hip folds them, then relabelled as vjp_flat.hip relabels its
// own.  Continuity and induction are one launch each, momentum and energy two, split by output group as in vjp_mhd.hip.
// An instantiation that needs scratch is not built and its entry returns PRE_E_UNSUPPORTED before any launch: modes 3 and
// 4 serve all four equations, mode 2 those of VJPFLATMHD_MODE2_* (the table: DESIGN 4.21, re-measure with resources.sh
// when a functor or the march changes).  A workgroup's LDS image is 2 * FIN * (512 + 64) * 16 B: 92 160 B at five streams.
#define VF_MAXIN 5
#define VF_MAXOUT 4
#define PRE_VJPFLAT_NO_ENTRIES 1
#include "vjp_flat.hip"
#include "../../include/cp_pre_vjpflatmhd.h"

// is the general-star instantiation of an equation built?  (momentum, energy: both passes; pass B of either needs scratch
// with general stars - 128 and 20 bytes)
#ifndef VJPFLATMHD_MODE2_CONTINUITY
#define VJPFLATMHD_MODE2_CONTINUITY 1
#endif
#ifndef VJPFLATMHD_MODE2_INDUCTION
#define VJPFLATMHD_MODE2_INDUCTION 1
#endif
#ifndef VJPFLATMHD_MODE2_MOMENTUM
#define VJPFLATMHD_MODE2_MOMENTUM 0
#endif
#ifndef VJPFLATMHD_MODE2_ENERGY
#define VJPFLATMHD_MODE2_ENERGY 0
#endif

namespace {

constexpr bool MODE2_BUILT[4] = {VJPFLATMHD_MODE2_CONTINUITY != 0, VJPFLATMHD_MODE2_MOMENTUM != 0, VJPFLATMHD_MODE2_ENERGY != 0,
                                 VJPFLATMHD_MODE2_INDUCTION != 0};      // by PRE_VJPMHD_EQ_*

struct Stars { Star Dt, Dx, Dy; int mode; };

// the three operators of an equation (on the caller's logical axes) and the tap structure they fit after the relabelling,
// chosen as the forward march chooses it; PRE_E_UNSUPPORTED for weight off the star or for a structure whose
// instantiation is not built
int stars_of(int eq, const float *K_t, const float *K_x, const float *K_y, Stars *s)
{
    if (!K_t || !K_x || !K_y) return PRE_E_NULL;
    if (!star_from_dense27(K_t, &s->Dt) || !star_from_dense27(K_x, &s->Dx) || !star_from_dense27(K_y, &s->Dy))
        return PRE_E_UNSUPPORTED;
    s->mode = relabeled_mode(pick_mode(s->Dt, s->Dx, s->Dy, nullptr), 1);
    return (s->mode == 2 && !MODE2_BUILT[eq]) ? PRE_E_UNSUPPORTED : PRE_OK;
}

const Star ZERO{0, 0, 0, 0, 0, 0, 0};
Star plus(const Star &a, const Star &b) { return combine(1.0, a, 1.0, b); }
Star minus(const Star &a, const Star &b) { return combine(1.0, a, -1.0, b); }
Star twice(const Star &a) { return combine(2.0, a, 0.0, ZERO); }
Star rl(const Star &s) { return relabelled(s); }

VjpMHDStars plain_stars(const Stars &s)
{
    return VjpMHDStars{rl(mirrored(s.Dt)), rl(s.Dx), rl(s.Dy), rl(mirrored(s.Dx)), rl(mirrored(s.Dy))};
}

// g and the nf fields in, the nf gradients out
struct Views {
    const pre_field_t *fs[7];
    const pre_out_t *os[6];
};

// every view of the entry checked once, all of them against each other, whichever launch reads them
int check_all(Views &v, const pre_field_t *g, const pre_field_t *fields, const pre_out_t *out, int nf, int64_t B, int64_t T,
              int64_t X, int64_t Y, int flags)
{
    v.fs[0] = g;
    for (int i = 0; i < nf; ++i) { v.fs[1 + i] = &fields[i]; v.os[i] = &out[i]; }
    return check_vjp_flat(v.fs, 1 + nf, v.os, nf, B, T, X, Y, flags);
}

// the geometry of one launch: streams `in` (0 is g) and outputs `out` of the checked views
int pass_of(FVGeom &g, const Views &v, const int *in, int nin, const int *out, int nout, int64_t B, int64_t T, int64_t X,
            int64_t Y, int flags, float host_scale, const float *dev_scale)
{
    const pre_field_t *fs[VF_MAXIN];
    const pre_out_t *os[VF_MAXOUT];
    for (int i = 0; i < nin; ++i) fs[i] = v.fs[in[i]];
    for (int k = 0; k < nout; ++k) os[k] = v.os[out[k]];
    return prepare_vjp_flat(g, fs, nin, os, nout, B, T, X, Y, flags, host_scale, dev_scale);
}

template <template <int> class Fn, bool MODE2>
int launch_mode(int mode, FVGeom &g, const typename Fn<2>::Params &p, hipStream_t st)
{
    static_assert(std::is_same<typename Fn<2>::Params, typename Fn<3>::Params>::value &&
                  std::is_same<typename Fn<2>::Params, typename Fn<4>::Params>::value, "one Params for every MODE");
    static_assert(Fn<2>::FIN <= VF_MAXIN && Fn<2>::FOUT <= VF_MAXOUT, "streams of a launch");
    if (mode == 3) return launch_vjp_flat<Fn<3>>(g, p, st);
    if (mode == 4) return launch_vjp_flat<Fn<4>>(g, p, st);
    if constexpr (MODE2) return launch_vjp_flat<Fn<2>>(g, p, st);
    return PRE_E_UNSUPPORTED;                            // (not reached: stars_of has declined)
}

}  // namespace

extern "C" {

int pre_vjpflatmhd_abi_version(void) { return PRE_VJPFLATMHD_ABI_VERSION; }

int pre_vjpflatmhd_supported(int eq, const float *K_t, const float *K_x, const float *K_y)
{
    if (eq < 0 || eq > 3) return PRE_E_RANGE;
    Stars s;
    return stars_of(eq, K_t, K_x, K_y, &s);
}

int pre_vjpflatmhd_continuity_f32(const pre_field_t *g, const pre_field_t fields[3], const pre_out_t out[3], const float *K_t,
                                  const float *K_x, const float *K_y, float host_scale, const float *dev_scale, int64_t B,
                                  int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !out || !K_t || !K_x || !K_y) return PRE_E_NULL;
    Views v;
    Stars s;
    FVGeom vg;
    int rc = check_all(v, g, fields, out, 3, B, T, X, Y, flags);
    if (rc) return rc;
    if ((rc = stars_of(PRE_VJPMHD_EQ_CONTINUITY, K_t, K_x, K_y, &s))) return rc;
    const int in[4] = {0, 1, 2, 3}, o[3] = {0, 1, 2};
    if ((rc = pass_of(vg, v, in, 4, o, 3, B, T, X, Y, flags, host_scale, dev_scale))) return rc;
    return launch_mode<VjpMHDContinuity, VJPFLATMHD_MODE2_CONTINUITY != 0>(s.mode, vg, plain_stars(s), as_stream(stream));
}

int pre_vjpflatmhd_induction_f32(const pre_field_t *g, const pre_field_t fields[4], const pre_out_t out[4], const float *K_t,
                                 const float *K_x, const float *K_y, float host_scale, const float *dev_scale, int64_t B,
                                 int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !out || !K_t || !K_x || !K_y) return PRE_E_NULL;
    Views v;
    Stars s;
    FVGeom vg;
    int rc = check_all(v, g, fields, out, 4, B, T, X, Y, flags);
    if (rc) return rc;
    if ((rc = stars_of(PRE_VJPMHD_EQ_INDUCTION, K_t, K_x, K_y, &s))) return rc;
    const int in[5] = {0, 1, 2, 3, 4}, o[4] = {0, 1, 2, 3};
    if ((rc = pass_of(vg, v, in, 5, o, 4, B, T, X, Y, flags, host_scale, dev_scale))) return rc;
    const Star M = minus(s.Dx, s.Dy), P = plus(s.Dx, s.Dy);
    const VjpMHDInductionParams p{rl(mirrored(s.Dt)), rl(M), rl(P), rl(mirrored(M)), rl(mirrored(P))};
    return launch_mode<VjpMHDInduction, VJPFLATMHD_MODE2_INDUCTION != 0>(s.mode, vg, p, as_stream(stream));
}

int pre_vjpflatmhd_momentum_f32(const pre_field_t *g, const pre_field_t fields[6], const pre_out_t out[6], const float *K_t,
                                const float *K_x, const float *K_y, float host_scale, const float *dev_scale, int64_t B,
                                int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !out || !K_t || !K_x || !K_y) return PRE_E_NULL;
    Views v;
    Stars s;
    FVGeom a, b;
    int rc = check_all(v, g, fields, out, 6, B, T, X, Y, flags);
    if (rc) return rc;
    if ((rc = stars_of(PRE_VJPMHD_EQ_MOMENTUM, K_t, K_x, K_y, &s))) return rc;
    // streams of the checked views: 0 g, 1 rho, 2 u, 3 v, 4 p, 5 Bx, 6 By; outputs in the order of the fields
    const int inA[3] = {0, 2, 3}, outA[2] = {1, 2}, inB[5] = {0, 1, 4, 5, 6}, outB[4] = {0, 3, 4, 5};
    if ((rc = pass_of(a, v, inA, 3, outA, 2, B, T, X, Y, flags, host_scale, dev_scale))) return rc;
    if ((rc = pass_of(b, v, inB, 5, outB, 4, B, T, X, Y, flags, host_scale, dev_scale))) return rc;
    const Star P = plus(s.Dx, s.Dy), D2x = twice(s.Dx), D2y = twice(s.Dy);
    const VjpMHDMomentumBParams pb{rl(P), rl(mirrored(P)), rl(D2x), rl(D2y), rl(mirrored(D2x)), rl(mirrored(D2y))};
    hipStream_t st = as_stream(stream);
    if ((rc = launch_mode<VjpMHDMomentumA, VJPFLATMHD_MODE2_MOMENTUM != 0>(s.mode, a, plain_stars(s), st))) return rc;
    return launch_mode<VjpMHDMomentumB, VJPFLATMHD_MODE2_MOMENTUM != 0>(s.mode, b, pb, st);
}

int pre_vjpflatmhd_energy_f32(const pre_field_t *g, const pre_field_t fields[6], const pre_out_t out[6], const float *K_t,
                              const float *K_x, const float *K_y, double gamma, float host_scale, const float *dev_scale,
                              int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !out || !K_t || !K_x || !K_y) return PRE_E_NULL;
    Views v;
    Stars s;
    FVGeom a, b;
    int rc = check_all(v, g, fields, out, 6, B, T, X, Y, flags);
    if (rc) return rc;
    if ((rc = stars_of(PRE_VJPMHD_EQ_ENERGY, K_t, K_x, K_y, &s))) return rc;
    const int inA[4] = {0, 4, 5, 6}, outA[3] = {0, 1, 2}, inB[5] = {0, 2, 3, 5, 6}, outB[3] = {3, 4, 5};
    if ((rc = pass_of(a, v, inA, 4, outA, 3, B, T, X, Y, flags, host_scale, dev_scale))) return rc;
    if ((rc = pass_of(b, v, inB, 5, outB, 3, B, T, X, Y, flags, host_scale, dev_scale))) return rc;
    const VjpMHDStars ps = plain_stars(s);
    // "(gamma-2)" is a float64 Python scalar in the reference: rounded once, as pre_residual_mhd_f32 does
    const VjpMHDEnergyParams p{ps.DtT, ps.Dx, ps.Dy, ps.DxT, ps.DyT, (float)gamma, (float)(gamma - 2.0)};
    hipStream_t st = as_stream(stream);
    if ((rc = launch_mode<VjpMHDEnergyA, VJPFLATMHD_MODE2_ENERGY != 0>(s.mode, a, p, st))) return rc;
    return launch_mode<VjpMHDEnergyB, VJPFLATMHD_MODE2_ENERGY != 0>(s.mode, b, p, st);
}

}  // extern "C"
