// pair_march.hip - data-driven residual scores d = r(a) - r(b) in one streaming pass (libcp_pre_pair.so,
// include/cp_pre_pair.h).
//
// The march of star_march.h evaluates a functor of up to MAXF = 6 field views.  Paired<Fn> (paired_functor.h, shared with
// screen_pair.hip) is a functor of 2*Fn::F views:
// views [0, F) are the truth set, [F, 2F) the prediction set, and eval = Fn::eval(first half) - Fn::eval(second half).
// Every layout mode of the march (contiguous, vars[:, i] views, the Nt-fastest relabelling, the flat form, the general
// star) and every flag (ABS after the subtraction, INTERIOR_T, OUT_INTERIOR_T, HALO_X) comes with it unchanged.
//
// The file is compiled twice (Makefile).  PRE_PAIR_PART 1, with the fma contraction of every other kernel here: the
// stencil, linear2, NS momentum and MHD continuity entries.  PRE_PAIR_PART 2, without fma contraction: the Burgers entry -
// contracted, the compiler fused the two halves of Paired<Burgers> differently and minus == vars gave 1-ulp differences
// instead of 0; uncontracted it runs as fast (memory-bound), while the paired NS momentum loses 38 %.
#ifndef PRE_PAIR_PART
#error "PRE_PAIR_PART: 1 or 2 (see the Makefile)"
#endif
#include "star_march.h"
#include "paired_functor.h"
#include "../../include/cp_pre_pair.h"

namespace {

// launch_mode without the general-star instantiation where the paired functor does not fit the registers: the general-star
// Paired<NSMomentum<2>> and Paired<MHDContinuity<2>> need more than the 256 VGPRs a 512-thread workgroup leaves a wave and
// spill (12-24 bytes per lane); that tap structure / layout returns PRE_E_UNSUPPORTED and the caller runs two single-set
// passes instead.
template <template <int> class FnT, bool GENERAL, class P>
int launch_pair_mode(int mode, Geom &g, const P &prm, hipStream_t st)
{
    if (mode == 0) return launch<FnT<0>>(g, prm, st);
    if (mode == 1) return launch<FnT<1>>(g, prm, st);
    if (mode == 3) return launch<FnT<3>>(g, prm, st);
    if (mode == 4) return launch<FnT<4>>(g, prm, st);
    if constexpr (GENERAL) return launch<FnT<2>>(g, prm, st);
    return PRE_E_UNSUPPORTED;
}

template <int M> using PairedBurgers = Paired<Burgers<M>>;

// ---- the <= 3 columns of an odd-width contiguous axis the march leaves (the twin's generic tail) -----------------------
// Kernel frame of prepare(): y is the unit-stride axis.  Zero padding; only the taps of non-zero weight are read, as the
// generic kernel reads its tap list.
__global__ void pair_star_tail_kernel(const Geom g, const Star s, int y0, long long total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ny = g.Y - y0;
    const int y = y0 + (int)(i % ny);
    long long r = i / ny;
    const int x = (int)(r % g.X);
    r /= g.X;
    const int t = (int)(r % g.T);
    const int b = (int)(r / g.T);
    float v[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float *p = g.f[k] + (long long)b * g.sB[k];
        auto at = [&](float w, int tt, int xx, int yy) {
            if (w == 0.f || tt < 0 || tt >= g.T || xx < 0 || xx >= g.X || yy < 0 || yy >= g.Y) return 0.f;
            return w * p[(long long)tt * g.sT[k] + (long long)xx * g.sX[k] + yy];
        };
        v[k] = at(s.tm, t - 1, x, y) + at(s.xm, t, x - 1, y) + at(s.ym, t, x, y - 1) + at(s.c, t, x, y) +
               at(s.yp, t, x, y + 1) + at(s.xp, t, x + 1, y) + at(s.tp, t + 1, x, y);
    }
    float d = v[0] - v[1];
    if (g.flags & PRE_FLAG_ABS) d = fabsf(d);
    g.out[(long long)b * g.oB + (long long)t * g.oT + (long long)x * g.oX + y] = d;
}

// PRE_E_SHAPE if `out` overlaps an input view (rows -1 and X included under PRE_FLAG_HALO_X for an input), or if a view's
// offsets leave int64
int check_disjoint(const pre_field_t *const *fs, int nf, const pre_out_t *out, int64_t B, int64_t T, int64_t X, int64_t Y,
                   int flags)
{
    const int64_t n[4] = {B, T, X, Y};
    const int64_t no[4] = {B, (flags & PRE_FLAG_OUT_INTERIOR_T) ? T - 2 : T, X, Y};
    const int64_t so[4] = {out->sB, out->sT, out->sX, out->sY};
    Span o, f;
    if (!span_of(out->ptr, so, no, 0, &o)) return PRE_E_SHAPE;
    for (int i = 0; i < nf; ++i) {
        const int64_t s[4] = {fs[i]->sB, fs[i]->sT, fs[i]->sX, fs[i]->sY};
        if (!span_of(fs[i]->ptr, s, n, (flags & PRE_FLAG_HALO_X) ? fs[i]->sX : 0, &f) || overlaps(o, f)) return PRE_E_SHAPE;
    }
    return PRE_OK;
}

// null / empty checks of everything the entry points dereference on the host, then the overlap check
int check_sets(const pre_field_t *const *fs, int nf, const pre_out_t *out, int64_t B, int64_t T, int64_t X, int64_t Y,
               int flags)
{
    if (!out || !out->ptr || B <= 0 || T <= 0 || X <= 0 || Y <= 0) return PRE_E_NULL;
    for (int i = 0; i < nf; ++i)
        if (!fs[i] || !fs[i]->ptr) return PRE_E_NULL;
    if ((flags & PRE_FLAG_OUT_INTERIOR_T) && T < 3) return PRE_E_UNSUPPORTED;
    return check_disjoint(fs, nf, out, B, T, X, Y, flags);
}

}  // namespace

extern "C" {

#if PRE_PAIR_PART == 1

int pre_pair_abi_version(void) { return PRE_PAIR_ABI_VERSION; }

int pre_pair_stencil3d_f32(const pre_field_t *a, const pre_field_t *b, const pre_out_t *out, const float *tap_w,
                           const int32_t *tap_off, int ntaps, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                           void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    if (flags & PRE_FLAG_OUT_INTERIOR_T) return PRE_E_UNSUPPORTED;          // (fused residual entries only, as the twin)
    const pre_field_t *fs[2] = {a, b};
    int rc = check_sets(fs, 2, out, B, T, X, Y, flags);
    if (rc) return rc;
    Linear1::Params p;
    if (!star_of_taps(tap_w, tap_off, ntaps, &p.s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    Star *stars[1] = {&p.s};
    Geom g;
    int rel;
    rc = prepare(g, rel, fs, 2, out, B, T, X, Y, flags, stars, 1, true);
    if (rc) return rc;
    g.tfree = no_t_taps(stars, 1);
    const int tail = g.Yc < g.Y ? g.Yc : -1;
    if (tail >= 0 && (flags & PRE_FLAG_HALO_X)) return PRE_E_UNSUPPORTED;   // (the tail pads x with zeros)
    if (tail >= 0) g.flags &= ~PRE_FLAG_INTERIOR_T;                          // (as the twin: every plane when a tail follows)
    hipStream_t st = as_stream(stream);
    if (g.Yc > 0) {
        rc = launch<Paired<Linear1>>(g, p, st);
        if (rc) return rc;
    }
    if (tail >= 0) {
        const long long total = (long long)g.B * g.T * g.X * (g.Y - tail);
        if ((total + 255) / 256 > 0x7fffffffLL) return PRE_E_SHAPE;
        hipLaunchKernelGGL(pair_star_tail_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, g, p.s, tail, total);
        PRE_LAUNCH_CHECK();
    }
    return PRE_OK;
}

int pre_pair_stencil2d_f32(const float *a, const int64_t a_strides[3], const float *b, const int64_t b_strides[3], float *out,
                           const int64_t out_strides[3], const float *tap_w, const int32_t *tap_off, int ntaps, int64_t B,
                           int64_t T, int64_t X, int flags, void *stream)
{
    if (!a || !a_strides || !b || !b_strides || !out || !out_strides || ntaps < 0 || (ntaps > 0 && !tap_off)) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    if (flags & PRE_FLAG_HALO_X) return PRE_E_UNSUPPORTED;                   // (the kernel's row axis is the caller's Nt here)
    // [B,T,X] with taps (dt,dx)  ==  [1,B,T,X] with taps (0,dt,dx), as pre_stencil2d_f32
    int32_t off3[3 * 343];
    for (int i = 0; i < ntaps; ++i) {
        off3[3 * i] = 0;
        off3[3 * i + 1] = tap_off[2 * i];
        off3[3 * i + 2] = tap_off[2 * i + 1];
    }
    pre_field_t fa{a, 0, a_strides[0], a_strides[1], a_strides[2]}, fb{b, 0, b_strides[0], b_strides[1], b_strides[2]};
    pre_out_t o{out, 0, out_strides[0], out_strides[1], out_strides[2]};
    return pre_pair_stencil3d_f32(&fa, &fb, &o, tap_w, off3, ntaps, 1, B, T, X, flags, stream);
}

int pre_pair_linear2_f32(const pre_field_t a[2], const pre_field_t b[2], const pre_out_t *out, const float *K_a,
                         const float *K_b, float ratio, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!a || !b || !K_a || !K_b) return PRE_E_NULL;
    const pre_field_t *fs[4] = {&a[0], &a[1], &b[0], &b[1]};
    int rc = check_sets(fs, 4, out, B, T, X, Y, flags);
    if (rc) return rc;
    Linear2::Params prm;
    if (!star_from_dense27(K_a, &prm.a) || !star_from_dense27(K_b, &prm.b)) return PRE_E_UNSUPPORTED;
    Star *stars[2] = {&prm.a, &prm.b};
    Geom g;
    int rel;
    rc = prepare(g, rel, fs, 4, out, B, T, X, Y, flags, stars, 2);
    if (rc) return rc;
    prm.ratio = ratio;
    g.tfree = no_t_taps(stars, 2);
    return launch<Paired<Linear2>>(g, prm, as_stream(stream));
}

int pre_pair_ns_momentum_f32(const pre_field_t a[3], const pre_field_t b[3], const pre_out_t *out, const float *K_t,
                             const float *K_x, const float *K_y, const float *K_xx_yy, float dt, float dx, float dy, float nu,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!a || !b || !K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    const pre_field_t *fs[6] = {&a[0], &a[1], &a[2], &b[0], &b[1], &b[2]};
    int rc = check_sets(fs, 6, out, B, T, X, Y, flags);
    if (rc) return rc;
    NSParams prm;
    int mode;
    rc = ns_params(prm, &mode, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu);
    if (rc) return rc;
    Star *stars[4] = {&prm.Dt, &prm.Dx, &prm.Dy, &prm.L};
    Geom g;
    int rel;
    rc = prepare(g, rel, fs, 6, out, B, T, X, Y, flags, stars, 4);
    if (rc) return rc;
    g.tfree = no_t_taps(stars, 4);
    return launch_pair_mode<PairedNS, false>(relabeled_mode(mode, rel), g, prm, as_stream(stream));
}

int pre_pair_mhd_continuity_f32(const pre_field_t a[3], const pre_field_t b[3], const pre_out_t *out, const float *K_t,
                                const float *K_x, const float *K_y, double gamma, int64_t B, int64_t T, int64_t X, int64_t Y,
                                int flags, void *stream)
{
    if (!a || !b || !K_t || !K_x || !K_y) return PRE_E_NULL;
    const pre_field_t *fs[6] = {&a[0], &a[1], &a[2], &b[0], &b[1], &b[2]};
    int rc = check_sets(fs, 6, out, B, T, X, Y, flags);
    if (rc) return rc;
    MHDParams prm;
    int mode;
    rc = mhd_params(prm, &mode, K_t, K_x, K_y, gamma);
    if (rc) return rc;
    Star *stars[3] = {&prm.Dt, &prm.Dx, &prm.Dy};
    Geom g;
    int rel;
    rc = prepare(g, rel, fs, 6, out, B, T, X, Y, flags, stars, 3);
    if (rc) return rc;
    g.tfree = no_t_taps(stars, 3);
    return launch_pair_mode<PairedMHDContinuity, false>(relabeled_mode(mode, rel), g, prm, as_stream(stream));
}

#endif  // PRE_PAIR_PART == 1
#if PRE_PAIR_PART == 2

int pre_pair_burgers_f32(const float *a, const int64_t a_strides[3], const float *b, const int64_t b_strides[3], float *out,
                         const int64_t out_strides[3], const float *K_t, const float *K_x, const float *K_xx, float dx, float dt,
                         float nu, float c3, int64_t B, int64_t T, int64_t X, int flags, void *stream)
{
    if (!a || !a_strides || !b || !b_strides || !out || !out_strides || !K_t || !K_x || !K_xx) return PRE_E_NULL;
    if (flags & (PRE_FLAG_OUT_INTERIOR_T | PRE_FLAG_HALO_X)) return PRE_E_UNSUPPORTED;     // (as the twin)
    // [B,T,X] -> [1, B, T, X]; 3x3 kernel (a over Nt, b over Nx) -> dense27 index (1, a, b), as pre_residual_burgers_f32
    pre_field_t fa{a, 0, a_strides[0], a_strides[1], a_strides[2]}, fb{b, 0, b_strides[0], b_strides[1], b_strides[2]};
    pre_out_t o{out, 0, out_strides[0], out_strides[1], out_strides[2]};
    const pre_field_t *fs[2] = {&fa, &fb};
    int rc = check_sets(fs, 2, &o, 1, B, T, X, flags);
    if (rc) return rc;
    float d27[3][27] = {};
    const float *k9[3] = {K_t, K_x, K_xx};
    for (int op = 0; op < 3; ++op)
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) d27[op][(1 * 3 + i) * 3 + c] = k9[op][i * 3 + c];
    BurgersParams prm;
    if (!star_from_dense27(d27[0], &prm.Dt) || !star_from_dense27(d27[1], &prm.Dx) || !star_from_dense27(d27[2], &prm.Dxx))
        return PRE_E_UNSUPPORTED;
    const Shape s0 = shape_of(prm.Dt), s1 = shape_of(prm.Dx), s2 = shape_of(prm.Dxx);
    const int mode = (!s0.y && !s1.x && !s2.x) ? 0 : 2;
    Star *stars[3] = {&prm.Dt, &prm.Dx, &prm.Dxx};
    Geom g;
    int rel;
    rc = prepare(g, rel, fs, 2, &o, 1, B, T, X, flags, stars, 3);
    if (rc) return rc;
    prm.dx = dx; prm.dt = dt; prm.nu = nu; prm.c3 = c3;
    g.tfree = no_t_taps(stars, 3);
    return launch_pair_mode<PairedBurgers, true>(rel == 0 ? mode : (rel == 2 && mode == 0 ? 3 : 2), g, prm, as_stream(stream));
}

#endif  // PRE_PAIR_PART == 2

}  // extern "C"
