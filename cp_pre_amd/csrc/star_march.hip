// star_march.hip - the entry points of libcp_pre_hip.so on the march of star_march.h: star stencils, the fused PDE residuals
// and the 2-D spatial operators with boundary conditions (gfx950 only).
#include "star_march.h"

// Internal: called by stencil_generic.hip when a tap list is star-shaped and the layout allows it.
// On success *tail_axis / *tail_from describe the columns the streaming kernel did NOT compute (the last
// extent % 4 cells of the contiguous axis, given as the caller's axis 0=T,1=X,2=Y and first index), or
// *tail_axis = -1 if everything was computed.
int pre_star_try_linear1(const pre_field_t *in, const pre_out_t *out, const float star7[7],
                         int64_t B, int64_t T, int64_t X, int64_t Y, int flags, hipStream_t st,
                         int *tail_axis, int64_t *tail_from)
{
    const pre_field_t *fs[1] = {in};
    Linear1::Params p;
    p.s = Star{star7[0], star7[1], star7[2], star7[3], star7[4], star7[5], star7[6]};
    Star *stars[1] = {&p.s};
    Geom g;
    int rel;
    int rc = prepare(g, rel, fs, 1, out, B, T, X, Y, flags, stars, 1, true);
    if (rc) return rc;
    *tail_axis = -1;
    g.tfree = no_t_taps(stars, 1);
    if (g.Yc < g.Y && (flags & PRE_FLAG_HALO_X)) return PRE_E_UNSUPPORTED;      // (the tail pass pads x with zeros)
    if (g.Yc < g.Y) {
        *tail_axis = rel == 0 ? 2 : (rel == 1 ? 0 : 1);
        *tail_from = g.Yc;
        g.flags &= ~PRE_FLAG_INTERIOR_T;           // keep it simple: the tail pass computes every plane
    }
    return launch<Linear1>(g, p, st);
}

extern "C" {

int pre_residual_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p, const pre_out_t *out,
                                 const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                 float dt, float dx, float dy, float nu,
                                 int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    const pre_field_t *fs[3] = {u, v, p};
    NSParams prm;
    int mode;
    int rc = ns_params(prm, &mode, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu);
    if (rc) return rc;
    Star *stars[4] = {&prm.Dt, &prm.Dx, &prm.Dy, &prm.L};
    Geom g;
    int rel;
    rc = prepare(g, rel, fs, 3, out, B, T, X, Y, flags, stars, 4);
    if (rc) return rc;
    g.tfree = no_t_taps(stars, 4);
    return launch_mode<NSMomentum>(relabeled_mode(mode, rel), g, prm, as_stream(stream));
}

int pre_residual_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const pre_out_t *out,
                             const float *K_a, const float *K_b, float ratio,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_a || !K_b) return PRE_E_NULL;
    const pre_field_t *fs[2] = {f0, f1};
    Linear2::Params prm;
    if (!star_from_dense27(K_a, &prm.a) || !star_from_dense27(K_b, &prm.b)) return PRE_E_UNSUPPORTED;
    Star *stars[2] = {&prm.a, &prm.b};
    Geom g;
    int rel;
    int rc = prepare(g, rel, fs, 2, out, B, T, X, Y, flags, stars, 2);
    if (rc) return rc;
    prm.ratio = ratio;
    g.tfree = no_t_taps(stars, 2);
    return launch<Linear2>(g, prm, as_stream(stream));
}

int pre_residual_burgers_f32(const float *u, const int64_t in_strides[3], float *out, const int64_t out_strides[3],
                             const float *K_t, const float *K_x, const float *K_xx,
                             float dx, float dt, float nu, float c3,
                             int64_t B, int64_t T, int64_t X, int flags, void *stream)
{
    if (!u || !in_strides || !out || !out_strides || !K_t || !K_x || !K_xx) return PRE_E_NULL;
    if (flags & (PRE_FLAG_OUT_INTERIOR_T | PRE_FLAG_HALO_X)) return PRE_E_UNSUPPORTED;     // [B,T,X]: the marched axis is the batch
    // [B,T,X] -> [1, B, T, X]; 3x3 kernel (a over Nt, b over Nx) -> dense27 index (1, a, b)
    pre_field_t f{u, 0, in_strides[0], in_strides[1], in_strides[2]};
    pre_out_t o{out, 0, out_strides[0], out_strides[1], out_strides[2]};
    const pre_field_t *fs[1] = {&f};
    float d27[3][27] = {};
    const float *k9[3] = {K_t, K_x, K_xx};
    for (int op = 0; op < 3; ++op)
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) d27[op][(1 * 3 + a) * 3 + c] = k9[op][a * 3 + c];
    BurgersParams prm;
    if (!star_from_dense27(d27[0], &prm.Dt) || !star_from_dense27(d27[1], &prm.Dx) || !star_from_dense27(d27[2], &prm.Dxx))
        return PRE_E_UNSUPPORTED;
    // mode 0 needs D_t purely along Nt (our x) and D_x, D_xx purely along Nx (our y)
    const Shape a = shape_of(prm.Dt), b2 = shape_of(prm.Dx), c2 = shape_of(prm.Dxx);
    const int mode = (!a.y && !b2.x && !c2.x) ? 0 : 2;
    Star *stars[3] = {&prm.Dt, &prm.Dx, &prm.Dxx};
    Geom g;
    int rel;
    int rc = prepare(g, rel, fs, 1, &o, 1, B, T, X, flags, stars, 3);
    if (rc) return rc;
    prm.dx = dx; prm.dt = dt; prm.nu = nu; prm.c3 = c3;
    g.tfree = no_t_taps(stars, 3);             // (always: the marched axis of [1,B,T,X] is the batch)
    return launch_mode<Burgers>(rel == 0 ? mode : (rel == 2 && mode == 0 ? 3 : 2), g, prm, as_stream(stream));
}

int pre_residual_mhd_f32(int eq, const pre_field_t fields[6], const pre_out_t *out,
                         const float *K_t, const float *K_x, const float *K_y, double gamma,
                         int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !K_t || !K_x || !K_y) return PRE_E_NULL;
    if (eq < 0 || eq > 3) return PRE_E_RANGE;
    MHDParams prm;
    int mode;
    int rc = mhd_params(prm, &mode, K_t, K_x, K_y, gamma);
    if (rc) return rc;
    const pre_field_t *all[6] = {&fields[0], &fields[1], &fields[2], &fields[3], &fields[4], &fields[5]};
    Star *stars[3] = {&prm.Dt, &prm.Dx, &prm.Dy};
    Geom g;
    int rel;
    hipStream_t st = as_stream(stream);
    if (eq == 0) {
        const pre_field_t *fs[3] = {all[0], all[1], all[2]};
        rc = prepare(g, rel, fs, 3, out, B, T, X, Y, flags, stars, 3);
        if (rc) return rc;
        g.tfree = no_t_taps(stars, 3);
        return launch_mode<MHDContinuity>(relabeled_mode(mode, rel), g, prm, st);
    }
    if (eq == 3) {
        const pre_field_t *fs[4] = {all[1], all[2], all[4], all[5]};
        rc = prepare(g, rel, fs, 4, out, B, T, X, Y, flags, stars, 3);
        if (rc) return rc;
        g.tfree = no_t_taps(stars, 3);
        return launch_mode<MHDInduction>(relabeled_mode(mode, rel), g, prm, st);
    }
    rc = prepare(g, rel, all, 6, out, B, T, X, Y, flags, stars, 3);
    if (rc) return rc;
    g.tfree = no_t_taps(stars, 3);
    if (eq == 1) return launch_mode<MHDMomentum>(relabeled_mode(mode, rel), g, prm, st);
    return launch_mode<MHDEnergy>(relabeled_mode(mode, rel), g, prm, st);
}

int pre_residual_jorek_f32(int eq, const pre_field_t fields[3], const pre_field_t *Rb, const pre_out_t *out,
                           const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                           const float coef[4], int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !Rb || !K_t || !K_R || !K_Z || !K_RR || !K_ZZ || !coef) return PRE_E_NULL;
    if (eq < 0 || eq > 1) return PRE_E_RANGE;
    JorekParams prm;
    int mode;
    int rc = jorek_params(prm, &mode, K_t, K_R, K_Z, K_RR, K_ZZ, coef);
    if (rc) return rc;
    Star *stars[5] = {&prm.Dt, &prm.DR, &prm.DZ, &prm.DRR, &prm.DZZ};
    Geom g;
    int rel;
    hipStream_t st = as_stream(stream);
    if (eq == 0) {
        const pre_field_t *fs[3] = {&fields[0], &fields[1], Rb};
        rc = prepare(g, rel, fs, 3, out, B, T, X, Y, flags, stars, 5);
        if (rc) return rc;
        g.tfree = no_t_taps(stars, 5);
        return launch_mode<JorekContinuity>(relabeled_mode(mode, rel), g, prm, st);
    }
    const pre_field_t *fs[4] = {&fields[0], &fields[1], &fields[2], Rb};
    rc = prepare(g, rel, fs, 4, out, B, T, X, Y, flags, stars, 5);
    if (rc) return rc;
    g.tfree = no_t_taps(stars, 5);
    return launch_mode<JorekTemperature>(relabeled_mode(mode, rel), g, prm, st);
}

// ---- 2-D spatial operators with boundary conditions ----------------------------
namespace {
int fill_bc(const pre_bc_t *bc, int64_t X, int64_t Y, BCInfo *o)
{
    if (!bc) return PRE_E_NULL;
    return bc_info(bc, X, Y, o) ? PRE_OK : PRE_E_RANGE;
}

bool star_from_dense9(const float *K, Star *s)     // 3x3 kernel, axes (X, Y)
{
    if (K[0] != 0.f || K[2] != 0.f || K[6] != 0.f || K[8] != 0.f) return false;
    *s = Star{K[4], 0.f, 0.f, K[1], K[7], K[3], K[5]};
    return true;
}
}  // namespace

int pre_spatial2d_bc_f32(const float *in, const int64_t in_strides[3], float *out, const int64_t out_strides[3],
                         const float *K, const pre_bc_t *bc, int64_t B, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!in || !out || !in_strides || !out_strides || !K) return PRE_E_NULL;
    if (flags & (PRE_FLAG_OUT_INTERIOR_T | PRE_FLAG_HALO_X)) return PRE_E_UNSUPPORTED;
    // planes [B,X,Y] -> [1,B,X,Y]: the plane axis is the tap-free marching axis
    pre_field_t f{in, 0, in_strides[0], in_strides[1], in_strides[2]};
    pre_out_t o{out, 0, out_strides[0], out_strides[1], out_strides[2]};
    if (f.sY != 1 || o.sY != 1) return PRE_E_UNSUPPORTED;            // no relabelling here: the BCs are tied to the axes
    const pre_field_t *fs[1] = {&f};
    Linear1::Params prm;
    if (!star_from_dense9(K, &prm.s)) return PRE_E_UNSUPPORTED;
    BCInfo info;
    int rc = fill_bc(bc, X, Y, &info);
    if (rc) return rc;
    Geom g;
    int rel;
    rc = prepare(g, rel, fs, 1, &o, 1, B, X, Y, flags & ~PRE_FLAG_INTERIOR_T, nullptr, 0, false, false);
    if (rc) return rc;
    g.tfree = 1;                               // (a 2-D operator: the marched axis is the batch of planes)
    return launch<Linear1, true>(g, prm, as_stream(stream), &info);
}

int pre_spatial2d_linear2_bc_f32(const float *in0, const int64_t s0[3], const float *in1, const int64_t s1[3], float *out,
                                 const int64_t out_strides[3], const float *K0, const float *K1, float ratio,
                                 const pre_bc_t *bc, int64_t B, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!in0 || !in1 || !out || !s0 || !s1 || !out_strides || !K0 || !K1) return PRE_E_NULL;
    if (flags & (PRE_FLAG_OUT_INTERIOR_T | PRE_FLAG_HALO_X)) return PRE_E_UNSUPPORTED;
    pre_field_t f0{in0, 0, s0[0], s0[1], s0[2]}, f1{in1, 0, s1[0], s1[1], s1[2]};
    pre_out_t o{out, 0, out_strides[0], out_strides[1], out_strides[2]};
    if (f0.sY != 1 || f1.sY != 1 || o.sY != 1) return PRE_E_UNSUPPORTED;
    const pre_field_t *fs[2] = {&f0, &f1};
    Linear2::Params prm;
    if (!star_from_dense9(K0, &prm.a) || !star_from_dense9(K1, &prm.b)) return PRE_E_UNSUPPORTED;
    prm.ratio = ratio;
    BCInfo info;
    int rc = fill_bc(bc, X, Y, &info);
    if (rc) return rc;
    Geom g;
    int rel;
    rc = prepare(g, rel, fs, 2, &o, 1, B, X, Y, flags & ~PRE_FLAG_INTERIOR_T, nullptr, 0, false, false);
    if (rc) return rc;
    g.tfree = 1;
    return launch<Linear2, true>(g, prm, as_stream(stream), &info);
}

}  // extern "C"
