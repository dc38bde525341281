// vjp_functors.h - what the backward passes of the residual losses share: the functors of the tiled march (vjp_march.h:
// residual_vjp.hip, libcp_pre_vjp.so; vjp_mhd.hip, libcp_pre_vjpmhd.so) and of the merged-row march (vjp_flat.hip,
// libcp_pre_vjpflat.so; vjp_flat_mhd.hip, libcp_pre_vjpflatmhd.so), the crop bits and the host-side folding of their stars.  With D(f)(x) = sum_k w_k f(x+k) (zero padding), D^T(g)(x) = sum_k w_k g(x-k): the same star with mirrored
// taps.  Every functor gets its stars already mirrored and folded with their scalar factors (host, in double, rounded once)
// and, in the merged-row march, relabelled to the kernel's axes.
#pragma once
#include "star_march.h"
#include "../../include/cp_pre_vjp.h"

namespace {

enum { CROP_T = 1, CROP_X = 2, CROP_Y = 4 };       // axes whose first and last cell the loss does not average over

__device__ __forceinline__ float4 mul4(const float4 &a, const float4 &b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ Nbr mul_nbr(const Nbr &a, const Nbr &b)
{
    return Nbr{mul4(a.c, b.c), mul4(a.tm, b.tm), mul4(a.tp, b.tp), mul4(a.xm, b.xm), mul4(a.xp, b.xp), mul4(a.ym, b.ym), mul4(a.yp, b.yp)};
}

// ------------------------------------------------------------------ the functors: n[0] is gg, r[] the gradients
struct VjpLinear1 {      // df = S^T(gg)
    static constexpr int FIN = 1, FOUT = 1;
    struct Params { Star st; };
    static __device__ __forceinline__ void eval(const Nbr (&n)[1], const Params &p, float4 (&r)[1]) { r[0] = apply<K_STAR7>(p.st, n[0]); }
};

struct VjpLinear2 {      // r = Sa(a) + ratio*Sb(b):  da = Sa^T(gg), db = ratio*Sb^T(gg)  (ratio folded into bt)
    static constexpr int FIN = 1, FOUT = 2;
    struct Params { Star at, bt; };
    static __device__ __forceinline__ void eval(const Nbr (&n)[1], const Params &p, float4 (&r)[2])
    {
        r[0] = apply<K_STAR7>(p.at, n[0]);
        r[1] = apply<K_STAR7>(p.bt, n[0]);
    }
};

// NS momentum, a = dx*dy, b = dt*dy, c = dt*dx, n = nu*dt (cp_pre_vjp.h):
//   du = (a*Dt^T - n*L^T)(gg) + gg*(b*Dx(u) + c*Dx(v)) + b*Dx^T(gg*u) + c*Dy^T(gg*v)
//   dv = (a*Dt^T - n*L^T)(gg) + gg*(c*Dy(u) + b*Dy(v)) + c*Dx^T(gg*u) + b*Dy^T(gg*v)
//   dp = (b*Dx^T + c*Dy^T)(gg)
struct VjpNSMomentum {
    static constexpr int FIN = 3, FOUT = 3;
    struct Params { Star lin, pT, Dx, Dy, DxT, DyT; float b, c; };     // lin = a*Dt^T - n*L^T, pT = b*Dx^T + c*Dy^T
    static __device__ __forceinline__ void eval(const Nbr (&n)[3], const Params &p, float4 (&r)[3])
    {
        const Nbr &g = n[0], &u = n[1], &v = n[2];
        const Nbr gu = mul_nbr(g, u), gv = mul_nbr(g, v);
        const float4 lin = apply<K_STAR7>(p.lin, g);
        const float4 X = apply<K_STAR7>(p.DxT, gu), Yv = apply<K_STAR7>(p.DyT, gv);
        r[0] = lin + mul4(g.c, p.b * apply<K_STAR7>(p.Dx, u) + p.c * apply<K_STAR7>(p.Dx, v)) + p.b * X + p.c * Yv;
        r[1] = lin + mul4(g.c, p.c * apply<K_STAR7>(p.Dy, u) + p.b * apply<K_STAR7>(p.Dy, v)) + p.c * X + p.b * Yv;
        r[2] = apply<K_STAR7>(p.pT, g);
    }
};

// ------------------------------------------------------------------ ideal MHD (vjp_mhd.hip, include/cp_pre_vjpmhd.h)
// The functors are templated on the MODE of the forward march (star_march.h: OpKinds, pick_mode), so that an operator
// multiplies only the taps its tap structure has; a mirrored star keeps its kind.  M = D_x - D_y and P = D_x + D_y are
// folded on the host and live on the union of the two structures: (Nt, Nx) in MODE 0, (Nx, Ny) in MODE 1; on the kernel
// axes of an Nt-fastest view (vjp_flat_mhd.hip) the marched axis and y in MODE 3, the marched axis and x in MODE 4.  With general
// stars everywhere (MODE 2) the one-pass forms need scratch; momentum and energy are split by output group into two
// launches whatever the MODE (the resource table: DESIGN 4.19).
template <int MODE> struct VjpKinds : OpKinds<MODE> {
    static constexpr int MP = MODE == 0 ? K_TX5 : MODE == 1 ? K_XY5 : MODE == 3 ? K_TY5 : MODE == 4 ? K_TX5 : K_STAR7;
};

template <class F> __device__ __forceinline__ Nbr nbr_of(const Nbr &a, const Nbr &b, F f)
{
    return Nbr{f(a.c, b.c), f(a.tm, b.tm), f(a.tp, b.tp), f(a.xm, b.xm), f(a.xp, b.xp), f(a.ym, b.ym), f(a.yp, b.yp)};
}
__device__ __forceinline__ Nbr add_nbr(const Nbr &a, const Nbr &b)
{
    return nbr_of(a, b, [](const float4 &x, const float4 &y) { return x + y; });
}

// continuity, r = Dt(rho) + u*Dx(rho) + rho*Dx(u) + v*Dy(rho) + rho*Dy(v); streams g, rho, u, v -> d rho, du, dv:
//   d rho = Dt^T g + Dx^T(g u) + Dy^T(g v) + g (Dx u + Dy v),  du = g Dx rho + Dx^T(g rho),  dv = g Dy rho + Dy^T(g rho)
struct VjpMHDStars { Star DtT, Dx, Dy, DxT, DyT; };
template <int MODE>
struct VjpMHDContinuity {
    static constexpr int FIN = 4, FOUT = 3;
    using Params = VjpMHDStars;
    static __device__ __forceinline__ void eval(const Nbr (&n)[4], const Params &p, float4 (&r)[3])
    {
        using K = VjpKinds<MODE>;
        const Nbr &g = n[0], &rho = n[1], &u = n[2], &v = n[3];
        const Nbr gu = mul_nbr(g, u), gv = mul_nbr(g, v), gr = mul_nbr(g, rho);
        r[0] = apply<K::DT>(p.DtT, g) + apply<K::DX>(p.DxT, gu) + apply<K::DY>(p.DyT, gv) +
               mul4(g.c, apply<K::DX>(p.Dx, u) + apply<K::DY>(p.Dy, v));
        r[1] = mul4(g.c, apply<K::DX>(p.Dx, rho)) + apply<K::DX>(p.DxT, gr);
        r[2] = mul4(g.c, apply<K::DY>(p.Dy, rho)) + apply<K::DY>(p.DyT, gr);
    }
};

// induction; streams g, u, v, Bx, By -> du, dv, dBx, dBy:
//   du  =  M^T(g By) + g P(By)          dv  = -M^T(g Bx) - g P(Bx)
//   dBx = Dt^T g - g M(v) - P^T(g v)    dBy = Dt^T g + g M(u) + P^T(g u)
struct VjpMHDInductionParams { Star DtT, M, P, MT, PT; };
template <int MODE>
struct VjpMHDInduction {
    static constexpr int FIN = 5, FOUT = 4;
    using Params = VjpMHDInductionParams;
    static __device__ __forceinline__ void eval(const Nbr (&n)[5], const Params &p, float4 (&r)[4])
    {
        using K = VjpKinds<MODE>;
        const Nbr &g = n[0], &u = n[1], &v = n[2], &bx = n[3], &by = n[4];
        const Nbr gu = mul_nbr(g, u), gv = mul_nbr(g, v), gbx = mul_nbr(g, bx), gby = mul_nbr(g, by);
        const float4 t = apply<K::DT>(p.DtT, g);
        r[0] = apply<K::MP>(p.MT, gby) + mul4(g.c, apply<K::MP>(p.P, by));
        r[1] = -(apply<K::MP>(p.MT, gbx) + mul4(g.c, apply<K::MP>(p.P, bx)));
        r[2] = t - mul4(g.c, apply<K::MP>(p.M, v)) - apply<K::MP>(p.PT, gv);
        r[3] = t + mul4(g.c, apply<K::MP>(p.M, u)) + apply<K::MP>(p.PT, gu);
    }
};

// momentum, with q = 1/rho, sx = 2 Dx Bx + P By, sy = 2 Dy By + P Bx, S = Bx sx + By sy:
//   r = Dt(u+v) + u Dx(u+v) + v Dy(u+v) + q (P p - S)
// pass A; streams g, u, v -> du, dv:   T = Dt^T g + Dx^T(g u) + Dy^T(g v),  du = T + g Dx(u+v),  dv = T + g Dy(u+v)
template <int MODE>
struct VjpMHDMomentumA {
    static constexpr int FIN = 3, FOUT = 2;
    using Params = VjpMHDStars;
    static __device__ __forceinline__ void eval(const Nbr (&n)[3], const Params &p, float4 (&r)[2])
    {
        using K = VjpKinds<MODE>;
        const Nbr &g = n[0], &u = n[1], &v = n[2];
        const Nbr gu = mul_nbr(g, u), gv = mul_nbr(g, v), w = add_nbr(u, v);
        const float4 t = apply<K::DT>(p.DtT, g) + apply<K::DX>(p.DxT, gu) + apply<K::DY>(p.DyT, gv);
        r[0] = t + mul4(g.c, apply<K::DX>(p.Dx, w));
        r[1] = t + mul4(g.c, apply<K::DY>(p.Dy, w));
    }
};

// g q at a neighbour.  Outside the view g is 0 and rho is the zero padding: the product there is 0, not 0 * inf - a select
// on exactly that pair of values (a cell inside the view with rho == 0 and g == 0 is taken the same way; a NaN or an inf
// in either is multiplied as it is).
__device__ __forceinline__ float gq1(float g, float rho) { return (g == 0.f && rho == 0.f) ? 0.f : g * (1.f / rho); }
__device__ __forceinline__ float4 gq4(const float4 &g, const float4 &rho)
{
    return make_float4(gq1(g.x, rho.x), gq1(g.y, rho.y), gq1(g.z, rho.z), gq1(g.w, rho.w));
}

// pass B; streams g, rho, p, Bx, By -> d rho, dp, dBx, dBy  (D2x = 2 Dx, D2y = 2 Dy, folded on the host):
//   d rho = -g q^2 (P p - S)                            dp  = P^T(g q)
//   dBx = -( g q sx + D2x^T(g q Bx) + P^T(g q By) )     dBy = -( g q sy + D2y^T(g q By) + P^T(g q Bx) )
struct VjpMHDMomentumBParams { Star P, PT, D2x, D2y, D2xT, D2yT; };
template <int MODE>
struct VjpMHDMomentumB {
    static constexpr int FIN = 5, FOUT = 4;
    using Params = VjpMHDMomentumBParams;
    static __device__ __forceinline__ void eval(const Nbr (&n)[5], const Params &p, float4 (&r)[4])
    {
        using K = VjpKinds<MODE>;
        const Nbr &g = n[0], &rho = n[1], &pr = n[2], &bx = n[3], &by = n[4];
        Nbr gq = nbr_of(g, rho, [](const float4 &a, const float4 &b) { return gq4(a, b); });
        const float4 q = f4(1.f) / rho.c;
        gq.c = mul4(g.c, q);
        const Nbr gqbx = mul_nbr(gq, bx), gqby = mul_nbr(gq, by);
        const float4 sx = apply<K::DX>(p.D2x, bx) + apply<K::MP>(p.P, by);
        const float4 sy = apply<K::DY>(p.D2y, by) + apply<K::MP>(p.P, bx);
        const float4 S = mul4(bx.c, sx) + mul4(by.c, sy);
        r[0] = -mul4(mul4(gq.c, q), apply<K::MP>(p.P, pr) - S);
        r[1] = apply<K::MP>(p.PT, gq);
        r[2] = -(mul4(gq.c, sx) + apply<K::DX>(p.D2xT, gqbx) + apply<K::MP>(p.PT, gqby));
        r[3] = -(mul4(gq.c, sy) + apply<K::DY>(p.D2yT, gqby) + apply<K::MP>(p.PT, gqbx));
    }
};

// energy, with pg = p - (Bx^2 + By^2)/2, A = gamma pg + By^2, C = gamma pg + Bx^2, E = Bx By, W = u Bx + v By,
// dv = Dx Bx + Dy By, sh = Dy u + Dx v, k = gamma - 2:
//   r = Dt(rho) + u Dx p + v Dy p + k W dv + A Dx u + C Dy v - E sh            (rho is not read: d rho = Dt^T g)
// pass A; streams g, p, Bx, By -> d rho, du, dv:
//   du = g (Dx p + k Bx dv) + Dx^T(g A) - Dy^T(g E)      dv = g (Dy p + k By dv) + Dy^T(g C) - Dx^T(g E)
struct VjpMHDEnergyParams { Star DtT, Dx, Dy, DxT, DyT; float gamma, k; };
template <int MODE>
struct VjpMHDEnergyA {
    static constexpr int FIN = 4, FOUT = 3;
    using Params = VjpMHDEnergyParams;
    static __device__ __forceinline__ void eval(const Nbr (&n)[4], const Params &p, float4 (&r)[3])
    {
        using K = VjpKinds<MODE>;
        const Nbr &g = n[0], &pr = n[1], &bx = n[2], &by = n[3];
        const float gamma = p.gamma;
        const Nbr bx2 = mul_nbr(bx, bx), by2 = mul_nbr(by, by);
        const Nbr gpg = nbr_of(pr, add_nbr(bx2, by2), [gamma](const float4 &a, const float4 &b) { return gamma * (a - 0.5f * b); });
        const Nbr gA = mul_nbr(g, add_nbr(gpg, by2)), gC = mul_nbr(g, add_nbr(gpg, bx2)), gE = mul_nbr(g, mul_nbr(bx, by));
        const float4 dv = apply<K::DX>(p.Dx, bx) + apply<K::DY>(p.Dy, by);
        r[0] = apply<K::DT>(p.DtT, g);
        r[1] = mul4(g.c, apply<K::DX>(p.Dx, pr) + p.k * mul4(bx.c, dv)) + apply<K::DX>(p.DxT, gA) - apply<K::DY>(p.DyT, gE);
        r[2] = mul4(g.c, apply<K::DY>(p.Dy, pr) + p.k * mul4(by.c, dv)) + apply<K::DY>(p.DyT, gC) - apply<K::DX>(p.DxT, gE);
    }
};

// pass B; streams g, u, v, Bx, By -> dp, dBx, dBy:
//   dp  = Dx^T(g u) + Dy^T(g v) + gamma g (Dx u + Dy v)
//   dBx = k (g u dv + Dx^T(g W)) + g ( Bx((2-gamma) Dy v - gamma Dx u) - By sh )
//   dBy = k (g v dv + Dy^T(g W)) + g ( By((2-gamma) Dx u - gamma Dy v) - Bx sh )
template <int MODE>
struct VjpMHDEnergyB {
    static constexpr int FIN = 5, FOUT = 3;
    using Params = VjpMHDEnergyParams;
    static __device__ __forceinline__ void eval(const Nbr (&n)[5], const Params &p, float4 (&r)[3])
    {
        using K = VjpKinds<MODE>;
        const Nbr &g = n[0], &u = n[1], &v = n[2], &bx = n[3], &by = n[4];
        const Nbr gu = mul_nbr(g, u), gv = mul_nbr(g, v);
        const Nbr gW = add_nbr(mul_nbr(gu, bx), mul_nbr(gv, by));
        const float4 dxu = apply<K::DX>(p.Dx, u), dyv = apply<K::DY>(p.Dy, v);
        const float4 dv = apply<K::DX>(p.Dx, bx) + apply<K::DY>(p.Dy, by);
        const float4 sh = apply<K::DY>(p.Dy, u) + apply<K::DX>(p.Dx, v);
        r[0] = apply<K::DX>(p.DxT, gu) + apply<K::DY>(p.DyT, gv) + p.gamma * mul4(g.c, dxu + dyv);
        r[1] = p.k * (mul4(gu.c, dv) + apply<K::DX>(p.DxT, gW)) +
               mul4(g.c, mul4(bx.c, -p.k * dyv - p.gamma * dxu) - mul4(by.c, sh));
        r[2] = p.k * (mul4(gv.c, dv) + apply<K::DY>(p.DyT, gW)) +
               mul4(g.c, mul4(by.c, -p.k * dxu - p.gamma * dyv) - mul4(bx.c, sh));
    }
};

// ------------------------------------------------------------------ host side
Star mirrored(const Star &s) { return Star{s.c, s.tp, s.tm, s.xp, s.xm, s.yp, s.ym}; }

// ca*a + cb*b, folded in double and rounded once
Star combine(double ca, const Star &a, double cb, const Star &b)
{
    auto m = [&](float x, float y) { return (float)(ca * (double)x + cb * (double)y); };
    return Star{m(a.c, b.c), m(a.tm, b.tm), m(a.tp, b.tp), m(a.xm, b.xm), m(a.xp, b.xp), m(a.ym, b.ym), m(a.yp, b.yp)};
}

// every view given, every extent positive
bool vjp_views_given(const pre_field_t *const *fs, int nf, const pre_out_t *const *os, int no, int64_t B, int64_t T, int64_t X,
                     int64_t Y)
{
    if (B <= 0 || T <= 0 || X <= 0 || Y <= 0) return false;
    for (int i = 0; i < nf; ++i)
        if (!fs[i] || !fs[i]->ptr) return false;
    for (int k = 0; k < no; ++k)
        if (!os[k] || !os[k]->ptr) return false;
    return true;
}

// No output's bounding byte range overlaps that of an input (or leaves the address space); the outputs among themselves
// may interleave (the slots of one stacked gradient tensor) but may not start at the same address.
bool vjp_views_disjoint(const pre_field_t *const *fs, int nf, const pre_out_t *const *os, int no, int64_t B, int64_t T, int64_t X,
                        int64_t Y)
{
    const int64_t n[4] = {B, T, X, Y};
    for (int k = 0; k < no; ++k) {
        const int64_t so[4] = {os[k]->sB, os[k]->sT, os[k]->sX, os[k]->sY};
        Span o, f;
        if (!span_of(os[k]->ptr, so, n, 0, &o)) return false;
        for (int i = 0; i < nf; ++i) {
            const int64_t s[4] = {fs[i]->sB, fs[i]->sT, fs[i]->sX, fs[i]->sY};
            if (!span_of(fs[i]->ptr, s, n, 0, &f) || overlaps(o, f)) return false;
        }
        for (int j = 0; j < k; ++j)
            if (os[j]->ptr == os[k]->ptr) return false;
    }
    return true;
}

int crop_of(int flags, bool view3d)
{
    if (!(flags & PRE_VJP_CROP)) return 0;
    return view3d ? (CROP_X | CROP_Y) : (CROP_T | CROP_X | CROP_Y);     // [B,T,X] is marched as [1,B,T,X]
}

}  // namespace
