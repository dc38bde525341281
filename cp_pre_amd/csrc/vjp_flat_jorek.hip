// vjp_flat_jorek.hip - the vector-Jacobian products of the reduced-MHD (JOREK) residuals for Nt-fastest views
// (libcp_pre_vjpjorek.so, include/cp_pre_vjpjorek.h): the backward pass of a physics-informed loss on
// JOREK.residual_continuity / residual_temperature of the dense [BS,F,Nx,Ny,Nt] tensor Joint/JOREK_residuals_CP.py holds.
//
// Notation (star_march.h): X(f) = D_R f D_Z phi - D_R phi D_Z f,  Y(f) = D_RR f + (1/R) D_R f + D_ZZ f,  h = gg R,  D^T the
// mirrored star, padding zero, gg the masked, scaled incoming gradient (vjp_flat.hip).  With
// J(f; s) = D_R^T(h s D_Z f) - D_Z^T(h s D_R f)  (s = 1 where it is left out) and  Y^T = D_RR^T gg + (1/R) D_R^T gg + D_ZZ^T gg:
//   continuity   r = a0 D_t rho - a1 R X(rho) - a2 rho D_Z phi - a3 Y(rho)
//     d rho = a0 D_t^T gg - a1 J(phi) - a2 gg D_Z phi - a3 Y^T
//     d phi = a1 J(rho) - a2 D_Z^T(gg rho)
//   temperature  r = T D_t rho + rho D_t T - rho R X(T) + T R X(rho) + a0 rho T D_Z phi + a3 Y(T)
//     d rho = D_t^T(gg T) + gg D_t T - h X(T) + J(phi; T) + a0 gg T D_Z phi
//     d T   = gg D_t rho + D_t^T(gg rho) - J(phi; rho) + h X(rho) + a0 gg rho D_Z phi + a3 Y^T
//     d phi = J(T; rho) - J(rho; T) + a0 D_Z^T(gg rho T)
// R is a grid: no gradient.  a0..a3 are pre_residual_jorek_f32's four scalars.
//
// The march is vjp_flat.hip's - included below without its entry points - in geometry (marched axis = Nx, kernel x = Ny,
// kernel y = Nt, L = Ny*Nt merged), split (flat_chunk, pick_tseg), host checks, per-element row-end masks and the mask of gg
// on load.  The plane loop is new.  J applies a mirrored star to a field that is itself a derivative, so a cell reads phi at
// the four corners of the (R, Z) plane: the functors take, for rho, phi (and T), the 3 x 3 BOX of (marched plane m-1, m,
// m+1) x (y-1, y, y+1), and the star of gg.  Only the tap structure the reference constructs is built (MODE 3 of star_march.h
// after the relabelling): D_R / D_RR have their taps on the marched axis, D_t / D_Z / D_ZZ on kernel y.  No operator has a tap
// along kernel x then, which is what makes R's centre value enough - R varies along kernel x only, so (1/R) commutes with
// D_R^T and a y-neighbour's h is gg there times the centre R - and what shortens the halo: a y-neighbour is the ADJACENT
// cell of the merged row, so ONE halo quad per side of a chunk is staged (vjp_flat.hip stages ceil(Nt/4): its x-neighbours
// lie Nt cells away); flat_chunk is asked as there, so the split is the same.  A corner cell takes the row-end mask of the
// centre plane's y-neighbour (the same position in the row); a plane outside the view is zero.
//
// The ring.  The own quads of planes m-1, m, m+1 are in registers (and m+2 in flight) as in vjp_flat.hip; their
// y-neighbours across quad edges are not, so the LDS image holds all three planes at once: step m writes plane m+1 (own
// quad and halo quad, loaded one step earlier than in vjp_flat.hip), waits at ONE barrier and reads planes m-1, m, m+1.
// Every plane is written to LDS once and fetched from HBM once.  A ring of three images would race: a thread that has left
// step m writes plane m+2 into slot (m+2) mod 3 = (m-1) mod 3 before the next barrier, while a slower thread may still read
// plane m-1 there.  With FOUR images the slot written in step m+2, (m+3) mod 4 = (m-1) mod 4, was last read in step m; a
// thread reaches the writes of step m+2 only through barrier m+1, at which every thread has arrived, step m's reads done.
// gg is read from LDS at plane m only and could do with two images; it rides in the same ring of four (one loop over the
// streams; the 16 KB do not change the residency, one workgroup per CU either way).  LDS: 4 x FIN x (512 + 2) quads =
// 98 688 B at three streams (continuity; d phi of temperature), 131 584 B at four (d rho, d T of temperature).
//
// Resources (csrc/resources.sh vjp_flat_jorek.hip): an instantiation with scratch in the plane loop is not
// built.  Temperature in ONE launch (VJPJOREK_TEMP_ONE_LAUNCH, off) needs 36 bytes of scratch at 256 VGPRs; it is TWO launches,
// split by output group as MHD momentum and energy are: (gg, rho, phi, T -> d rho, d T) and (gg, rho, T -> d phi), which
// does not read phi.  Both have scratch = 0, as has continuity.
#define VF_MAXIN 4
#define VF_MAXOUT 3
#define PRE_VJPFLAT_NO_ENTRIES 1
#include "vjp_flat.hip"
#include "../../include/cp_pre_vjpjorek.h"

#ifndef VJPJOREK_TEMP_ONE_LAUNCH
#define VJPJOREK_TEMP_ONE_LAUNCH 0
#endif

namespace {

constexpr int JH = 1;            // halo quads per side of a chunk: the y-neighbour is the adjacent cell of the merged row

// the 3 x 3 box of one stream: v[p][y], p = marched plane m-1, m, m+1, y = kernel y-1, y, y+1
struct Box { float4 v[3][3]; };

// On the kernel's axes: DtT, DZT, DZZT the mirrored stars (taps ym, c, yp), DRT, DRRT likewise (tm, c, tp).
struct JorekVjpParams {
    Star Dt, DR, DZ, DtT, DRT, DZT, DRRT, DZZT;
    float a0, a1, a2, a3;
    const float *R;              // [Ny][Nt]: the radius at every position of the merged row
};

struct JorekOps {
    const JorekVjpParams &p;
    // one tap: a zero weight is not multiplied (the centre of a first difference), so that a NaN under it reaches nothing -
    // the non-finite set of the gradient is the composed expression's.  The weights are wave-uniform.
    static __device__ __forceinline__ float4 tap(float w, const float4 &v) { return w != 0.f ? w * v : f4(0.f); }
    // a star with its taps along kernel y (ym, c, yp) / along the marched axis (tm, c, tp) on three values along that axis
    static __device__ __forceinline__ float4 y3(const Star &s, const float4 &a, const float4 &b, const float4 &c) { return tap(s.ym, a) + tap(s.c, b) + tap(s.yp, c); }
    static __device__ __forceinline__ float4 t3(const Star &s, const float4 &a, const float4 &b, const float4 &c) { return tap(s.tm, a) + tap(s.c, b) + tap(s.tp, c); }
    // along kernel y, at plane pl of a box
    __device__ __forceinline__ float4 dZ(const Box &b, int pl) const { return y3(p.DZ, b.v[pl][0], b.v[pl][1], b.v[pl][2]); }
    __device__ __forceinline__ float4 dt(const Box &b) const { return y3(p.Dt, b.v[1][0], b.v[1][1], b.v[1][2]); }
    // along the marched axis, at column y of a box
    __device__ __forceinline__ float4 dR(const Box &b, int y) const { return t3(p.DR, b.v[0][y], b.v[1][y], b.v[2][y]); }
    // J(f; s) / R = D_R^T(gg s D_Z f) - D_Z^T(gg s D_R f); s: a box of which the star is read
    __device__ __forceinline__ float4 J(const Box &g, const Box &f, const Box &s) const
    {
        const float4 r = t3(p.DRT, mul4(mul4(g.v[0][1], s.v[0][1]), dZ(f, 0)), mul4(mul4(g.v[1][1], s.v[1][1]), dZ(f, 1)),
                            mul4(mul4(g.v[2][1], s.v[2][1]), dZ(f, 2)));
        const float4 z = y3(p.DZT, mul4(mul4(g.v[1][0], s.v[1][0]), dR(f, 0)), mul4(mul4(g.v[1][1], s.v[1][1]), dR(f, 1)),
                            mul4(mul4(g.v[1][2], s.v[1][2]), dR(f, 2)));
        return r - z;
    }
    __device__ __forceinline__ float4 J(const Box &g, const Box &f) const
    {
        const float4 r = t3(p.DRT, mul4(g.v[0][1], dZ(f, 0)), mul4(g.v[1][1], dZ(f, 1)), mul4(g.v[2][1], dZ(f, 2)));
        const float4 z = y3(p.DZT, mul4(g.v[1][0], dR(f, 0)), mul4(g.v[1][1], dR(f, 1)), mul4(g.v[1][2], dR(f, 2)));
        return r - z;
    }
    // Y^T = D_RR^T gg + (1/R) D_R^T gg + D_ZZ^T gg
    __device__ __forceinline__ float4 YT(const Box &g, const float4 &R) const
    {
        return t3(p.DRRT, g.v[0][1], g.v[1][1], g.v[2][1]) + mul4(f4(1.0f) / R, t3(p.DRT, g.v[0][1], g.v[1][1], g.v[2][1])) +
               y3(p.DZZT, g.v[1][0], g.v[1][1], g.v[1][2]);
    }
    __device__ __forceinline__ float4 X(const Box &f, const Box &phi) const { return mul4(dR(f, 1), dZ(phi, 1)) - mul4(dR(phi, 1), dZ(f, 1)); }
};

// streams gg, rho, phi -> d rho, d phi
struct JorekVjpContinuity {
    static constexpr int FIN = 3, FOUT = 2;
    static __device__ __forceinline__ void eval(const Box (&b)[3], const float4 &R, const JorekVjpParams &p, float4 (&r)[2])
    {
        const JorekOps o{p};
        const Box &g = b[0], &rho = b[1], &phi = b[2];
        const float4 gc = g.v[1][1];
        r[0] = p.a0 * o.y3(p.DtT, g.v[1][0], gc, g.v[1][2]) - p.a1 * mul4(R, o.J(g, phi)) - p.a2 * mul4(gc, o.dZ(phi, 1)) - p.a3 * o.YT(g, R);
        r[1] = p.a1 * mul4(R, o.J(g, rho)) -
               p.a2 * o.y3(p.DZT, mul4(g.v[1][0], rho.v[1][0]), mul4(gc, rho.v[1][1]), mul4(g.v[1][2], rho.v[1][2]));
    }
};

// GROUP 0: streams gg, rho, phi, T -> d rho, d phi, d T (one launch); 1: the same streams -> d rho, d T; 2: gg, rho, T -> d phi
template <int GROUP>
struct JorekVjpTemperature {
    static constexpr int FIN = GROUP == 2 ? 3 : 4, FOUT = GROUP == 0 ? 3 : GROUP == 1 ? 2 : 1;
    static __device__ __forceinline__ void eval(const Box (&b)[FIN], const float4 &R, const JorekVjpParams &p, float4 (&r)[FOUT])
    {
        const JorekOps o{p};
        const Box &g = b[0], &rho = b[1], &T = b[FIN - 1];
        const float4 gc = g.v[1][1];
        if constexpr (GROUP != 2) {
            const Box &phi = b[2];
            const float4 h = mul4(gc, R);
            const float4 dZphi = o.dZ(phi, 1);
            const float4 drho = o.y3(p.DtT, mul4(g.v[1][0], T.v[1][0]), mul4(gc, T.v[1][1]), mul4(g.v[1][2], T.v[1][2])) + mul4(gc, o.dt(T)) -
                                mul4(h, o.X(T, phi)) + mul4(R, o.J(g, phi, T)) + p.a0 * mul4(mul4(gc, T.v[1][1]), dZphi);
            const float4 dT = mul4(gc, o.dt(rho)) + o.y3(p.DtT, mul4(g.v[1][0], rho.v[1][0]), mul4(gc, rho.v[1][1]), mul4(g.v[1][2], rho.v[1][2])) -
                              mul4(R, o.J(g, phi, rho)) + mul4(h, o.X(rho, phi)) + p.a0 * mul4(mul4(gc, rho.v[1][1]), dZphi) + p.a3 * o.YT(g, R);
            r[0] = drho;
            r[GROUP == 0 ? 2 : 1] = dT;
        }
        if constexpr (GROUP != 1) {
            const float4 grt0 = mul4(g.v[1][0], mul4(rho.v[1][0], T.v[1][0])), grt1 = mul4(gc, mul4(rho.v[1][1], T.v[1][1])),
                         grt2 = mul4(g.v[1][2], mul4(rho.v[1][2], T.v[1][2]));
            r[GROUP == 0 ? 1 : 0] = mul4(R, o.J(g, T, rho) - o.J(g, rho, T)) + p.a0 * o.y3(p.DZT, grt0, grt1, grt2);
        }
    }
};

// ------------------------------------------------------------------ the march: vjp_flat_kernel's, with the ring of planes
template <class Fn>
__global__ void __launch_bounds__(FLAT_NT) vjp_jorek_kernel(const FVGeom g, const JorekVjpParams prm)
{
    constexpr int F = Fn::FIN, FO = Fn::FOUT;
    __shared__ float4 lds[4][F][FLAT_NT + 2 * JH];
    const int q = threadIdx.x;
    unsigned Lb = xcd_remap(blockIdx.x, gridDim.x);
    const int ch = Lb % g.nCh; Lb /= g.nCh;
    const int ts = Lb % g.nTSeg;
    const int b = Lb / g.nTSeg;
    const int Ty = g.Y, L = g.X * g.Y;
    const int NT = blockDim.x;                     // threads per chunk, chosen by the host (the LDS image is sized for 512)
    const int t0 = ts * g.tSeg, t1 = min(t0 + g.tSeg, g.T);
    const float scale = g.scale * (g.dev_scale ? *g.dev_scale : 1.0f);

    const int m0 = ch * NT * 4, m = m0 + 4 * q;
    const bool inb = m < L;                        // (whole quads only: L % 4 == 0, checked by the host)

    // halo duty: the first / last thread fetches the quad left / right of the chunk
    const bool hl = q < JH, hr = q >= NT - JH;
    const int hm = hl ? m0 - 4 * (JH - q) : m0 + 4 * NT + 4 * (q - (NT - JH));
    const bool hok = (hl || hr) && hm >= 0 && hm < L;
    const int hslot = hl ? q : JH + NT + (q - (NT - JH));

    // per cell of my quad: its y- / y+ neighbour inside its own row, the loss's mask (vjp_flat.hip)
    bool lok[4], rok[4];
    unsigned kown = 0, khal = 0;
    {
        int ph = m % Ty, xr = m / Ty;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lok[j] = ph != 0;
            rok[j] = ph != Ty - 1;
            if (inb && xr >= g.crop && xr < g.X - g.crop && ph >= g.crop && ph < Ty - g.crop) kown |= 1u << j;
            if (++ph == Ty) { ph = 0; ++xr; }
        }
        if (hok) {
            ph = hm % Ty; xr = hm / Ty;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (xr >= g.crop && xr < g.X - g.crop && ph >= g.crop && ph < Ty - g.crop) khal |= 1u << j;
                if (++ph == Ty) { ph = 0; ++xr; }
            }
        }
    }
    auto keep_t = [&](int t) { return t >= g.crop && t < g.T - g.crop; };
    auto masked = [&](const float4 &v, unsigned k, bool kt) __attribute__((always_inline)) {
        return make_float4((kt && (k & 1u)) ? scale * v.x : 0.f, (kt && (k & 2u)) ? scale * v.y : 0.f,
                           (kt && (k & 4u)) ? scale * v.z : 0.f, (kt && (k & 8u)) ? scale * v.w : 0.f);
    };

    const unsigned int voff = (unsigned int)m * 4u, hoff = (unsigned int)hm * 4u;       // (hm < 0: never loaded)
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    auto quad_at = [&](const float *p, unsigned int off) __attribute__((always_inline)) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(__builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, -1, 0x00020000),
                                                              (int)off, 0, 0);
        return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    };
    auto quad = [&](int i, int t, unsigned int off) __attribute__((always_inline)) {
        return quad_at(g.f[i] + ((long long)b * g.sB[i] + (long long)t * g.sT[i]), off);
    };
    auto load_own = [&](int t, float4(&dst)[F]) __attribute__((always_inline)) {
        const bool ok = inb && (t >= 0) && (t < g.T);
#pragma unroll
        for (int i = 0; i < F; ++i) {
            if (ok) dst[i] = quad(i, t, voff);
            else dst[i] = f4(0.f);
            if (i == 0) dst[i] = masked(dst[i], kown, keep_t(t));
        }
    };
    auto load_halo = [&](int t, float4(&dst)[F]) __attribute__((always_inline)) {
        const bool ok = hok && (t >= 0) && (t < g.T);
#pragma unroll
        for (int i = 0; i < F; ++i) {
            if (ok) dst[i] = quad(i, t, hoff);
            else dst[i] = f4(0.f);
            if (i == 0) dst[i] = masked(dst[i], khal, keep_t(t));
        }
    };
    // plane t of every stream into its slot of the ring
    auto stage = [&](int t, const float4(&own)[F], const float4(&hal)[F]) __attribute__((always_inline)) {
        const int s = (t - t0 + 1) & 3;
#pragma unroll
        for (int i = 0; i < F; ++i) {
            lds[s][i][JH + q] = own[i];
            if (hl || hr) lds[s][i][hslot] = hal[i];
        }
    };

    // R at my four positions of the merged row: the same on every plane (1 where the thread owns nothing: 1/R)
    const float4 R = inb ? quad_at(prm.R, voff) : f4(1.0f);

    long long oo[FO];
#pragma unroll
    for (int k = 0; k < FO; ++k) oo[k] = (long long)b * g.oB[k] + m;

    // One plane.  P, C, N hold planes t-1, t, t+1 of the own quads, D receives plane t+2; hn is the halo quad of plane t+1,
    // hd receives that of plane t+2.  Planes t-1 and t are in the ring already.
    auto step = [&](int t, float4(&P)[F], float4(&C)[F], float4(&N)[F], float4(&D)[F], float4(&hn)[F], float4(&hd)[F])
                    __attribute__((always_inline)) {
        stage(t + 1, N, hn);
        load_halo(t + 2, hd);            // (consumed first: vmcnt retires in issue order)
        load_own(t + 2, D);
        lds_barrier();

        Box bx[F];
#pragma unroll
        for (int i = 0; i < F; ++i) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                const float4 &c = pl == 0 ? P[i] : pl == 1 ? C[i] : N[i];
                bx[i].v[pl][1] = c;
                if (i == 0 && pl != 1) continue;                   // (gg: its star only)
                const float *row = reinterpret_cast<const float *>(&lds[(t + pl - t0) & 3][i][0]) + 4 * (JH + q);      // my first cell
                const float lft = row[-1], rgt = row[4];
                bx[i].v[pl][0] = make_float4(lok[0] ? lft : 0.f, lok[1] ? c.x : 0.f, lok[2] ? c.y : 0.f, lok[3] ? c.z : 0.f);
                bx[i].v[pl][2] = make_float4(rok[0] ? c.y : 0.f, rok[1] ? c.z : 0.f, rok[2] ? c.w : 0.f, rok[3] ? rgt : 0.f);
            }
        }
        float4 r[FO];
        Fn::eval(bx, R, prm, r);
        if (inb) {
#pragma unroll
            for (int k = 0; k < FO; ++k) stg4(g.o[k] + oo[k] + (long long)t * g.oT[k], r[k]);
        }
    };

    float4 w0[F], w1[F], w2[F], w3[F], h0[F], h1[F];
    load_own(t0 - 1, w0);
    load_halo(t0 - 1, h0);
    load_own(t0, w1);
    load_halo(t0, h1);
    stage(t0 - 1, w0, h0);
    stage(t0, w1, h1);
    load_own(t0 + 1, w2);
    load_halo(t0 + 1, h0);
    for (int t = t0; t < t1; t += 4) {
        step(t, w0, w1, w2, w3, h0, h1);
        if (t + 1 >= t1) break;
        step(t + 1, w1, w2, w3, w0, h1, h0);
        if (t + 2 >= t1) break;
        step(t + 2, w2, w3, w0, w1, h0, h1);
        if (t + 3 >= t1) break;
        step(t + 3, w3, w0, w1, w2, h1, h0);
    }
}

// ------------------------------------------------------------------ host side
template <class Fn>
int launch_vjp_jorek(FVGeom &g, const JorekVjpParams &prm, hipStream_t st)
{
    static_assert(4 * Fn::FIN * (FLAT_NT + 2 * JH) * 16 <= 160 * 1024, "ring does not fit the 160 KiB LDS");
    static_assert(Fn::FIN <= VF_MAXIN && Fn::FOUT <= VF_MAXOUT, "streams of a launch");
    const long long quads = (long long)g.X * g.Y / 4;
    const int nt = flat_chunk(quads, g.Y, true);                   // (asked as vjp_flat.hip asks: the same split)
    g.nCh = (int)((quads + nt - 1) / nt);
    static std::atomic<int> per_cu[FLAT_NT / 64 + 1] = {};         // (by chunk width)
    unsigned grid;
    const int rc = flat_split(vjp_jorek_kernel<Fn>, nt, per_cu, g, (long long)g.B * g.nCh, g.T, &grid);
    if (rc) return rc;
    hipLaunchKernelGGL((vjp_jorek_kernel<Fn>), dim3(grid), dim3(nt), 0, st, g, prm);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}

// The five operators on the caller's axes -> the stars of the functors on the kernel's.  PRE_E_UNSUPPORTED for weight off
// the star and for every tap structure but the reference's construction (pre_residual_jorek_f32's choice of it: mode 0).
int jorek_stars(JorekVjpParams &p, const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ)
{
    if (!K_t || !K_R || !K_Z || !K_RR || !K_ZZ) return PRE_E_NULL;
    Star Dt, DR, DZ, DRR, DZZ;
    if (!star_from_dense27(K_t, &Dt) || !star_from_dense27(K_R, &DR) || !star_from_dense27(K_Z, &DZ) ||
        !star_from_dense27(K_RR, &DRR) || !star_from_dense27(K_ZZ, &DZZ))
        return PRE_E_UNSUPPORTED;
    const Shape rr = shape_of(DRR), zz = shape_of(DZZ);
    if (pick_mode(Dt, DR, DZ, nullptr) != 0 || rr.t || rr.y || zz.x || zz.y) return PRE_E_UNSUPPORTED;
    p.Dt = relabelled(Dt); p.DR = relabelled(DR); p.DZ = relabelled(DZ);
    p.DtT = relabelled(mirrored(Dt)); p.DRT = relabelled(mirrored(DR)); p.DZT = relabelled(mirrored(DZ));
    p.DRRT = relabelled(mirrored(DRR)); p.DZZT = relabelled(mirrored(DZZ));
    return PRE_OK;
}

}  // namespace

extern "C" {

int pre_vjpjorek_abi_version(void) { return PRE_VJPJOREK_ABI_VERSION; }

int pre_vjpjorek_supported(int eq, const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ)
{
    if (eq < 0 || eq > 1) return PRE_E_RANGE;
    JorekVjpParams p;
    return jorek_stars(p, K_t, K_R, K_Z, K_RR, K_ZZ);
}

int pre_vjpjorek_flat_f32(int eq, const pre_field_t *g, const pre_field_t fields[3], const pre_field_t *Rb, const pre_out_t out[3],
                          const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                          const float coef[4], float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X,
                          int64_t Y, int flags, void *stream)
{
    if (!fields || !Rb || !out || !K_t || !K_R || !K_Z || !K_RR || !K_ZZ || !coef) return PRE_E_NULL;
    if (eq < 0 || eq > 1) return PRE_E_RANGE;
    const int nf = 2 + eq;
    // g, rho, phi (, T), and R checked as an input too: null, and no output over it
    const pre_field_t *fs[5] = {g, &fields[0], &fields[1], nf == 3 ? &fields[2] : Rb, Rb};
    const pre_out_t *os[3] = {&out[0], &out[1], &out[2]};
    if (!Rb->ptr) return PRE_E_NULL;
    int rc = check_vjp_flat(fs, 1 + nf, os, nf, B, T, X, Y, flags);
    if (rc) return rc;
    // R repeats its row: a [Y][T] array behind every sample and plane (an axis of extent 1 may carry any stride)
    if ((T > 1 && Rb->sT != 1) || (Y > 1 && Rb->sY != T) || (X > 1 && Rb->sX != 0) || (B > 1 && Rb->sB != 0)) return PRE_E_UNSUPPORTED;
    if (!vjp_views_disjoint(fs + 4, 1, os, nf, B, T, X, Y)) return PRE_E_SHAPE;
    JorekVjpParams p;
    if ((rc = jorek_stars(p, K_t, K_R, K_Z, K_RR, K_ZZ))) return rc;
    p.a0 = coef[0]; p.a1 = coef[1]; p.a2 = coef[2]; p.a3 = coef[3];
    p.R = Rb->ptr;
    hipStream_t st = as_stream(stream);
    FVGeom vg;
    if (eq == 0) {
        if ((rc = prepare_vjp_flat(vg, fs, 3, os, 2, B, T, X, Y, flags, host_scale, dev_scale))) return rc;
        return launch_vjp_jorek<JorekVjpContinuity>(vg, p, st);
    }
    // outputs in the order of the fields: d rho, d phi, d T
#if VJPJOREK_TEMP_ONE_LAUNCH
    if ((rc = prepare_vjp_flat(vg, fs, 4, os, 3, B, T, X, Y, flags, host_scale, dev_scale))) return rc;
    return launch_vjp_jorek<JorekVjpTemperature<0>>(vg, p, st);
#else
    FVGeom vb;
    const pre_field_t *fb[3] = {g, &fields[0], &fields[2]};
    const pre_out_t *oa[2] = {&out[0], &out[2]}, *ob[1] = {&out[1]};
    if ((rc = prepare_vjp_flat(vg, fs, 4, oa, 2, B, T, X, Y, flags, host_scale, dev_scale))) return rc;
    if ((rc = prepare_vjp_flat(vb, fb, 3, ob, 1, B, T, X, Y, flags, host_scale, dev_scale))) return rc;
    if ((rc = launch_vjp_jorek<JorekVjpTemperature<1>>(vg, p, st))) return rc;
    return launch_vjp_jorek<JorekVjpTemperature<2>>(vb, p, st);
#endif
}

}  // extern "C"
