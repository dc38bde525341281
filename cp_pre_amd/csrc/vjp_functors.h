// vjp_functors.h - what the backward passes of the residual losses share: the functors of the tiled march (residual_vjp.hip,
// libcp_pre_vjp.so) and of the merged-row march (vjp_flat.hip, libcp_pre_vjpflat.so), the crop bits and the host-side folding
// of their stars.  With D(f)(x) = sum_k w_k f(x+k) (zero padding), D^T(g)(x) = sum_k w_k g(x-k): the same star with mirrored
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
