// residual_bc.hip - the entry points of libcp_pre_bcres.so: the fused residuals of star_march.hip under boundary conditions
// on the x-y rim (include/cp_pre_bcres.h).  No march of its own: the BC = true instantiations of star_march.h's march_kernel
// with the functors of the zero-pad passes, compiled with star_march.o's flags so that they round as those passes do.
//
// Out-of-range planes under BC.  With a tap along the marched axis the planes t = -1 and t = T must contribute zero
// everywhere, their padded ring included.  The fills the kernel gives such a plane (load_own: `ghost`, load_halo: hfill,
// efill, yrfill) are the sides' constants, not zero - and none of them reaches an output: the x / y taps of a star act on
// the centre plane only, which is never out of range (a step runs for t0 <= t < t1 <= T), LDS is staged from the centre
// plane only, and tm / tp read a thread's OWN cells, whose `ghost` is 0 for every thread that stores (it is the constant
// only in the ghost row x == X of a partial last tile, whose threads never store).
#include "star_march.h"
#include "../../include/cp_pre_bcres.h"

namespace {

// rows of the tile launch<Fn, true> picks for a width (star_march.h: launch)
inline int tile_rows(int64_t Y) { return Y >= 192 ? 8 : Y >= 96 ? 16 : 32; }

// What every entry checks before prepare(): flags, the layout the conditions are tied to, the conditions themselves, the
// 32-bit in-plane offsets.  fs / out: [B,T,X,Y] views (the 1-D family as [1,B,T,X]).
int bc_args(const pre_field_t *const *fs, int nf, const pre_out_t *out, const pre_bc_t *bc, int64_t B, int64_t T, int64_t X,
            int64_t Y, int flags, BCInfo *info)
{
    if (!bc || !out || !out->ptr || B <= 0 || T <= 0 || X <= 0 || Y <= 0) return PRE_E_NULL;
    for (int i = 0; i < nf; ++i)
        if (!fs[i] || !fs[i]->ptr) return PRE_E_NULL;
    if (flags & (PRE_FLAG_OUT_INTERIOR_T | PRE_FLAG_HALO_X)) return PRE_E_UNSUPPORTED;
    if (B > 0x7fffffff || T > 0x7fffffff || X > 0x7fffffff || Y > 0x7fffffff) return PRE_E_SHAPE;
    if (!bc_info(bc, X, Y, info)) return PRE_E_RANGE;
    if (out->sY != 1 || Y % 4 != 0) return PRE_E_UNSUPPORTED;          // no relabelling here: the BCs are tied to the axes
    for (int i = 0; i < nf; ++i)
        if (fs[i]->sY != 1) return PRE_E_UNSUPPORTED;
    for (int i = 0; i < nf; ++i)
        if (!plane_offsets_fit_u32(fs[i]->sX, X + 2 + tile_rows(Y), Y)) return PRE_E_RANGE;
    return PRE_OK;
}

// the three tap structures on the caller's axes (nothing is relabelled: modes 3 / 4 do not occur).  GENERAL = false: the
// general-star instantiation is not built and the entry declines - MHD momentum and energy, whose six views with the second
// edge scalar per field do not fit the register file (256 VGPRs and 44-92 bytes of scratch inside the plane loop,
// profiles/bcres/resources_all.txt; the tap structures of the reference's operators fit)
template <template <int> class FnT, bool GENERAL = true, class P>
int launch_mode_bc(int mode, Geom &g, const P &prm, hipStream_t st, const BCInfo *info)
{
    if (mode == 0) return launch<FnT<0>, true>(g, prm, st, info);
    if (mode == 1) return launch<FnT<1>, true>(g, prm, st, info);
    if constexpr (GENERAL) return launch<FnT<2>, true>(g, prm, st, info);
    return PRE_E_UNSUPPORTED;
}

// the 1-D family: the rows (time) of the [T,X] plane take the constant 0, the zero padding
pre_bc_t rows_bc(const pre_bc_t *bc)
{
    pre_bc_t r = *bc;
    r.mode[2] = r.mode[3] = PRE_BC_CONSTANT;
    r.value[2] = r.value[3] = 0.f;
    return r;
}

}  // namespace

extern "C" {

int pre_bcres_abi_version(void) { return PRE_BCRES_ABI_VERSION; }

int pre_bcres_linear1_f32(const pre_field_t *in, const pre_out_t *out, const float *K, const pre_bc_t *bc,
                          int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K) return PRE_E_NULL;
    const pre_field_t *fs[1] = {in};
    BCInfo info;
    int rc = bc_args(fs, 1, out, bc, B, T, X, Y, flags, &info);
    if (rc) return rc;
    Linear1::Params prm;
    if (!star_from_dense27(K, &prm.s)) return PRE_E_UNSUPPORTED;
    Star *stars[1] = {&prm.s};
    Geom g;
    int rel;
    rc = prepare(g, rel, fs, 1, out, B, T, X, Y, flags, stars, 1, false, false);
    if (rc) return rc;
    g.tfree = no_t_taps(stars, 1);
    return launch<Linear1, true>(g, prm, as_stream(stream), &info);
}

int pre_bcres_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const pre_out_t *out,
                          const float *K_a, const float *K_b, float ratio, const pre_bc_t *bc,
                          int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_a || !K_b) return PRE_E_NULL;
    const pre_field_t *fs[2] = {f0, f1};
    BCInfo info;
    int rc = bc_args(fs, 2, out, bc, B, T, X, Y, flags, &info);
    if (rc) return rc;
    Linear2::Params prm;
    if (!star_from_dense27(K_a, &prm.a) || !star_from_dense27(K_b, &prm.b)) return PRE_E_UNSUPPORTED;
    prm.ratio = ratio;
    Star *stars[2] = {&prm.a, &prm.b};
    Geom g;
    int rel;
    rc = prepare(g, rel, fs, 2, out, B, T, X, Y, flags, stars, 2, false, false);
    if (rc) return rc;
    g.tfree = no_t_taps(stars, 2);
    return launch<Linear2, true>(g, prm, as_stream(stream), &info);
}

int pre_bcres_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p, const pre_out_t *out,
                              const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                              float dt, float dx, float dy, float nu, const pre_bc_t *bc,
                              int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    const pre_field_t *fs[3] = {u, v, p};
    BCInfo info;
    int rc = bc_args(fs, 3, out, bc, B, T, X, Y, flags, &info);
    if (rc) return rc;
    NSParams prm;
    int mode;
    rc = ns_params(prm, &mode, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu);
    if (rc) return rc;
    Star *stars[4] = {&prm.Dt, &prm.Dx, &prm.Dy, &prm.L};
    Geom g;
    int rel;
    rc = prepare(g, rel, fs, 3, out, B, T, X, Y, flags, stars, 4, false, false);
    if (rc) return rc;
    g.tfree = no_t_taps(stars, 4);
    return launch_mode_bc<NSMomentum>(mode, g, prm, as_stream(stream), &info);
}

int pre_bcres_mhd_f32(int eq, const pre_field_t fields[6], const pre_out_t *out,
                      const float *K_t, const float *K_x, const float *K_y, double gamma, const pre_bc_t *bc,
                      int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !K_t || !K_x || !K_y) return PRE_E_NULL;
    if (eq < 0 || eq > 3) return PRE_E_RANGE;
    const pre_field_t *all[6] = {&fields[0], &fields[1], &fields[2], &fields[3], &fields[4], &fields[5]};
    BCInfo info;
    int rc = bc_args(all, 6, out, bc, B, T, X, Y, flags, &info);
    if (rc) return rc;
    MHDParams prm;
    int mode;
    rc = mhd_params(prm, &mode, K_t, K_x, K_y, gamma);
    if (rc) return rc;
    Star *stars[3] = {&prm.Dt, &prm.Dx, &prm.Dy};
    Geom g;
    int rel;
    hipStream_t st = as_stream(stream);
    if (eq == 0) {
        const pre_field_t *fs[3] = {all[0], all[1], all[2]};
        rc = prepare(g, rel, fs, 3, out, B, T, X, Y, flags, stars, 3, false, false);
        if (rc) return rc;
        g.tfree = no_t_taps(stars, 3);
        return launch_mode_bc<MHDContinuity>(mode, g, prm, st, &info);
    }
    if (eq == 3) {
        const pre_field_t *fs[4] = {all[1], all[2], all[4], all[5]};
        rc = prepare(g, rel, fs, 4, out, B, T, X, Y, flags, stars, 3, false, false);
        if (rc) return rc;
        g.tfree = no_t_taps(stars, 3);
        return launch_mode_bc<MHDInduction>(mode, g, prm, st, &info);
    }
    rc = prepare(g, rel, all, 6, out, B, T, X, Y, flags, stars, 3, false, false);
    if (rc) return rc;
    g.tfree = no_t_taps(stars, 3);
    if (eq == 1) return launch_mode_bc<MHDMomentum, false>(mode, g, prm, st, &info);
    return launch_mode_bc<MHDEnergy, false>(mode, g, prm, st, &info);
}

int pre_bcres_burgers_f32(const float *u, const int64_t in_strides[3], float *out, const int64_t out_strides[3],
                          const float *K_t, const float *K_x, const float *K_xx,
                          float dx, float dt, float nu, float c3, const pre_bc_t *bc,
                          int64_t B, int64_t T, int64_t X, int flags, void *stream)
{
    if (!u || !in_strides || !out || !out_strides || !K_t || !K_x || !K_xx || !bc) return PRE_E_NULL;
    // [B,T,X] -> [1, B, T, X]; 3x3 kernel (a over Nt, b over Nx) -> dense27 index (1, a, b)
    pre_field_t f{u, 0, in_strides[0], in_strides[1], in_strides[2]};
    pre_out_t o{out, 0, out_strides[0], out_strides[1], out_strides[2]};
    const pre_field_t *fs[1] = {&f};
    const pre_bc_t rb = rows_bc(bc);
    BCInfo info;
    int rc = bc_args(fs, 1, &o, &rb, 1, B, T, X, flags, &info);
    if (rc) return rc;
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
    rc = prepare(g, rel, fs, 1, &o, 1, B, T, X, flags & ~PRE_FLAG_INTERIOR_T, stars, 3, false, false);
    if (rc) return rc;
    prm.dx = dx; prm.dt = dt; prm.nu = nu; prm.c3 = c3;
    g.tfree = 1;                               // (the marched axis of [1,B,T,X] is the batch)
    if (mode == 0) return launch<Burgers<0>, true>(g, prm, as_stream(stream), &info);
    return launch<Burgers<2>, true>(g, prm, as_stream(stream), &info);
}

int pre_bcres_linear1_rows_f32(const float *in, const int64_t in_strides[3], float *out, const int64_t out_strides[3],
                               const float *K, const pre_bc_t *bc,
                               int64_t B, int64_t T, int64_t X, int flags, void *stream)
{
    if (!in || !in_strides || !out || !out_strides || !K || !bc) return PRE_E_NULL;
    pre_field_t f{in, 0, in_strides[0], in_strides[1], in_strides[2]};
    pre_out_t o{out, 0, out_strides[0], out_strides[1], out_strides[2]};
    const pre_field_t *fs[1] = {&f};
    const pre_bc_t rb = rows_bc(bc);
    BCInfo info;
    int rc = bc_args(fs, 1, &o, &rb, 1, B, T, X, flags, &info);
    if (rc) return rc;
    Cross k;
    if (!cross_from_dense9(K, &k)) return PRE_E_UNSUPPORTED;
    Linear1::Params prm;
    prm.s = Star{k.c, 0.f, 0.f, k.xm, k.xp, k.ym, k.yp};       // kernel axes (Nt, Nx) = the plane's (rows, columns)
    Geom g;
    int rel;
    rc = prepare(g, rel, fs, 1, &o, 1, B, T, X, flags & ~PRE_FLAG_INTERIOR_T, nullptr, 0, false, false);
    if (rc) return rc;
    g.tfree = 1;
    return launch<Linear1, true>(g, prm, as_stream(stream), &info);
}

}  // extern "C"
