// vjp_march.h - the tiled march of the backward passes of the residual losses (residual_vjp.hip: libcp_pre_vjp.so;
// vjp_mhd.hip: libcp_pre_vjpmhd.so): the kernel, its geometry, its launch and the host-side checks of its views.
//
// The march templates are star_march.h's (Star, Nbr, apply<>, the lane shifts, the LDS-only barrier, pick_tseg).
// The march of that header has ONE output stream and reads its inputs as stored; a gradient has several outputs, and the
// incoming gradient g has to be masked (the loss averages over the cropped interior) and scaled on load.  Hence a march of
// its own here, same structure: a workgroup of NR x TYQ threads owns NR rows x 4*TYQ columns of one sample and marches over
// t; every thread keeps planes t-1, t, t+1 (and the in-flight t+2) of its own quad per input stream in registers; the
// current plane goes through LDS (double-buffered, one barrier per plane) for the x-neighbours, halo rows included; the
// y-neighbours come from the adjacent lane, the two edge lanes of a row fetch one scalar.  Stream 0 is always g: what is
// kept in registers and LDS is gg = m ? scale * g : 0 (a select: a NaN outside the crop does not spread), so no masked or
// scaled copy of the residual ever exists in memory.  Widths that are no multiple of 4 are handled in the same launch: the
// last quad of a row loads and stores element by element.  Every other stream reads zero outside the view (the zero
// padding of the operators).
//
// A functor Fn: FIN input streams (n[0] is gg), FOUT output streams, Params, eval(n, params, r).
#pragma once
#include "vjp_functors.h"

namespace {

// the most streams a launch takes; the entries that split a gradient into two launches check the views of both at once
// (MHD momentum: g and six fields in, six gradients out)
constexpr int VJP_MAXIN = 7, VJP_MAXOUT = 6;

struct VGeom {
    const float *f[VJP_MAXIN];
    long long sB[VJP_MAXIN], sT[VJP_MAXIN], sX[VJP_MAXIN];
    float *o[VJP_MAXOUT];
    long long oB[VJP_MAXOUT], oT[VJP_MAXOUT], oX[VJP_MAXOUT];
    int B, T, X, Y;
    int tSeg, nTSeg, nXT, nYT;
    int crop;                    // CROP_* bits: axes whose first and last cell the loss does not average over
    int tfree;                   // no star has a tap along the marched axis: a segment loads its own planes only
    float scale;                 // host factor of g ...
    const float *dev_scale;      // ... times this device scalar, if given (the upstream gradient of loss.backward())
};

// ------------------------------------------------------------------ the march
template <int F> struct VHalo { float row[F], ye[F]; };

template <class Fn, int NR, int TYQ>
__global__ void __launch_bounds__(NR *TYQ) vjp_march_kernel(const VGeom g, const typename Fn::Params prm)
{
    constexpr int F = Fn::FIN, FO = Fn::FOUT;
    static_assert(NR >= 8 && (4 * TYQ) % 64 == 0 && NR * TYQ >= 8 * TYQ, "the two halo rows are fetched by the first 8*TYQ threads");
    __shared__ float4 lds[2][F][NR + 2][TYQ];

    const int q = threadIdx.x, ty = threadIdx.y;
    unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const int yt = L % g.nYT; L /= g.nYT;
    const int xt = L % g.nXT; L /= g.nXT;
    const int ts = L % g.nTSeg;
    const int b = L / g.nTSeg;

    const int x = xt * NR + ty, y = (yt * TYQ + q) * 4;
    const bool inb = (x < g.X) && (y < g.Y);
    const bool full = inb && (y + 3 < g.Y);              // (else: the row's last, partial quad - element by element)
    const int t0 = ts * g.tSeg, t1 = min(t0 + g.tSeg, g.T);
    const int tlo = g.tfree ? t0 : 0, thi = g.tfree ? t1 : g.T;
    const float scale = g.scale * (g.dev_scale ? *g.dev_scale : 1.0f);

    // the 0/1 mask of the loss on g, per axis
    const bool cT = g.crop & CROP_T, cX = g.crop & CROP_X, cY = g.crop & CROP_Y;
    auto keep_t = [&](int t) { return !cT || (t >= 1 && t <= g.T - 2); };
    auto keep_x = [&](int xx) { return !cX || (xx >= 1 && xx <= g.X - 2); };
    auto keep_y = [&](int yy) { return !cY || (yy >= 1 && yy <= g.Y - 2); };
    const bool kx = keep_x(x);
    const bool ky[4] = {kx && keep_y(y), kx && keep_y(y + 1), kx && keep_y(y + 2), kx && keep_y(y + 3)};

    // halo-row duty: the first 4*TYQ threads fetch the row above the tile, the next 4*TYQ the row below, a float each
    const int hl = ty * TYQ + q;
    const bool hduty = hl < 8 * TYQ, hbot = hl >= 4 * TYQ;
    const int hcol = hl & (4 * TYQ - 1);
    const int hy = yt * (4 * TYQ) + hcol;
    const int hx = hbot ? xt * NR + NR : xt * NR - 1;
    const bool hrow = hduty && hx >= 0 && hx < g.X && hy < g.Y;
    const bool hkeep = keep_x(hx) && keep_y(hy);
    const int hslot = hbot ? NR + 1 : 0;
    // y-halo duty: the first lane of a wave / row fetches its y- cell, the last lane its y+ cell
    const bool ledge = (q & 63) == 0, redge = ((q & 63) == 63) || (q == TYQ - 1);
    const int ey = ledge ? y - 1 : y + 4;
    const bool eload = inb && (ledge ? y > 0 : (redge && y + 4 < g.Y));
    const bool ekeep = kx && keep_y(ey);

    long long own[F], hal[F], edg[F];
#pragma unroll
    for (int i = 0; i < F; ++i) {
        const long long base = (long long)b * g.sB[i];
        own[i] = base + (long long)x * g.sX[i] + y;
        hal[i] = base + (long long)hx * g.sX[i] + hy;
        edg[i] = base + (long long)x * g.sX[i] + ey;
    }

    auto load_own = [&](int t, float4(&dst)[F]) __attribute__((always_inline)) {
        const bool okt = (t >= tlo) && (t < thi);
#pragma unroll
        for (int i = 0; i < F; ++i) {
            float4 v = f4(0.f);
            if (inb && okt) {
                const float *p = g.f[i] + own[i] + (long long)t * g.sT[i];
                if (full) {
                    v = ldg4(p);
                } else {
                    v.x = p[0];
                    if (y + 1 < g.Y) v.y = p[1];
                    if (y + 2 < g.Y) v.z = p[2];
                }
            }
            if (i == 0) {
                const bool kt = keep_t(t);
                v.x = (kt && ky[0]) ? scale * v.x : 0.f;
                v.y = (kt && ky[1]) ? scale * v.y : 0.f;
                v.z = (kt && ky[2]) ? scale * v.z : 0.f;
                v.w = (kt && ky[3]) ? scale * v.w : 0.f;
            }
            dst[i] = v;
        }
    };
    auto load_halo = [&](int t, VHalo<F> &h) __attribute__((always_inline)) {
        const bool okt = (t >= tlo) && (t < thi);
#pragma unroll
        for (int i = 0; i < F; ++i) {
            float r = (hrow && okt) ? g.f[i][hal[i] + (long long)t * g.sT[i]] : 0.f;
            float e = (eload && okt) ? g.f[i][edg[i] + (long long)t * g.sT[i]] : 0.f;
            if (i == 0) {
                const bool kt = keep_t(t);
                r = (kt && hkeep) ? scale * r : 0.f;
                e = (kt && ekeep) ? scale * e : 0.f;
            }
            h.row[i] = r;
            h.ye[i] = e;
        }
    };

    long long oo[FO];
#pragma unroll
    for (int k = 0; k < FO; ++k) oo[k] = (long long)b * g.oB[k] + (long long)x * g.oX[k] + y;

    // One plane.  P, C, N hold planes t-1, t, t+1 of the own quads, D receives plane t+2; hc is the halo of plane t, hn
    // receives that of plane t+1.  The caller rotates the roles instead of moving registers.
    auto step = [&](int t, float4(&P)[F], float4(&C)[F], float4(&N)[F], float4(&D)[F], VHalo<F> &hc, VHalo<F> &hn)
                    __attribute__((always_inline)) {
        const int bi = (t - t0) & 1;
#pragma unroll
        for (int i = 0; i < F; ++i) {
            lds[bi][i][ty + 1][q] = C[i];
            if (hduty) reinterpret_cast<float *>(&lds[bi][i][hslot][0])[hcol] = hc.row[i];
        }
        load_halo(t + 1, hn);            // (consumed first: vmcnt retires in issue order)
        load_own(t + 2, D);
        lds_barrier();

        Nbr n[F];
#pragma unroll
        for (int i = 0; i < F; ++i) {
            n[i].c = C[i];
            n[i].tm = P[i];
            n[i].tp = N[i];
            n[i].xm = lds[bi][i][ty][q];
            n[i].xp = lds[bi][i][ty + 2][q];
            float lft = lane_below(C[i].w);
            float rgt = lane_above(C[i].x);
            lft = ledge ? hc.ye[i] : lft;
            rgt = redge ? hc.ye[i] : rgt;
            n[i].ym = make_float4(lft, C[i].x, C[i].y, C[i].z);
            n[i].yp = make_float4(C[i].y, C[i].z, C[i].w, rgt);
        }
        float4 r[FO];
        Fn::eval(n, prm, r);
        if (inb) {
#pragma unroll
            for (int k = 0; k < FO; ++k) {
                float *p = g.o[k] + oo[k] + (long long)t * g.oT[k];
                if (full) {
                    stg4(p, r[k]);
                } else {
                    p[0] = r[k].x;
                    if (y + 1 < g.Y) p[1] = r[k].y;
                    if (y + 2 < g.Y) p[2] = r[k].z;
                }
            }
        }
    };

    VHalo<F> h0, h1;
    float4 w0[F], w1[F], w2[F], w3[F];
    load_own(t0 - 1, w0);
    load_own(t0, w1);
    load_own(t0 + 1, w2);
    load_halo(t0, h0);
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
template <class Fn, int NR, int TYQ>
int launch_vjp_tiled(VGeom &g, const typename Fn::Params &prm, hipStream_t st)
{
    static_assert(2 * Fn::FIN * (NR + 2) * TYQ * 16 <= 160 * 1024, "tile does not fit the 160 KiB LDS");
    g.nXT = (g.X + NR - 1) / NR;
    g.nYT = (g.Y + 4 * TYQ - 1) / (4 * TYQ);
    long long tiles = (long long)g.B * g.nXT * g.nYT;
    static const int per_cu = resident_per_cu(vjp_march_kernel<Fn, NR, TYQ>, NR * TYQ);
    int tSeg = pick_tseg(tiles, g.T, (long long)per_cu * chip_cus());
    if (g.tfree && tSeg > TFREE_TSEG) tSeg = TFREE_TSEG;          // (segments cost no window prologue then: star_march.h)
    g.tSeg = tSeg;
    g.nTSeg = (g.T + tSeg - 1) / tSeg;
    tiles *= g.nTSeg;
    if (tiles <= 0 || tiles * TYQ > 0xffffffffLL || tiles > 0x7fffffffLL) return PRE_E_SHAPE;
    hipLaunchKernelGGL((vjp_march_kernel<Fn, NR, TYQ>), dim3((unsigned)tiles), dim3(TYQ, NR), 0, st, g, prm);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}

template <class Fn>
int launch_vjp(VGeom &g, const typename Fn::Params &prm, hipStream_t st)
{
    if (g.Y >= 192) return launch_vjp_tiled<Fn, 8, 64>(g, prm, st);      // 8 rows x 256 columns, as the forward march
    return launch_vjp_tiled<Fn, 32, 16>(g, prm, st);                     // narrow grids: 32 rows x 64 columns
}

// Null / empty / layout / overlap checks of everything the entry points hand to a kernel, and the geometry.  Views that
// are not disjoint (vjp_functors.h) are PRE_E_SHAPE, as in pair_march.hip.
int prepare_vjp(VGeom &g, const pre_field_t *const *fs, int nf, const pre_out_t *const *os, int no, int64_t B, int64_t T,
                int64_t X, int64_t Y, int crop, float host_scale, const float *dev_scale)
{
    if (!vjp_views_given(fs, nf, os, no, B, T, X, Y)) return PRE_E_NULL;
    if (B > 0x7fffffff || T > 0x7fffffff || X > 0x7fffffff || Y > 0x7fffffff - 8) return PRE_E_SHAPE;
    for (int i = 0; i < nf; ++i)
        if (fs[i]->sY != 1) return PRE_E_UNSUPPORTED;              // (Nt-fastest views and the like: the caller falls back)
    for (int k = 0; k < no; ++k)
        if (os[k]->sY != 1) return PRE_E_UNSUPPORTED;
    if (!vjp_views_disjoint(fs, nf, os, no, B, T, X, Y)) return PRE_E_SHAPE;
    for (int i = 0; i < VJP_MAXIN; ++i) {
        const bool on = i < nf;
        g.f[i] = on ? fs[i]->ptr : nullptr;
        g.sB[i] = on ? fs[i]->sB : 0; g.sT[i] = on ? fs[i]->sT : 0; g.sX[i] = on ? fs[i]->sX : 0;
    }
    for (int k = 0; k < VJP_MAXOUT; ++k) {
        const bool on = k < no;
        g.o[k] = on ? os[k]->ptr : nullptr;
        g.oB[k] = on ? os[k]->sB : 0; g.oT[k] = on ? os[k]->sT : 0; g.oX[k] = on ? os[k]->sX : 0;
    }
    g.B = (int)B; g.T = (int)T; g.X = (int)X; g.Y = (int)Y;
    g.crop = crop;
    g.tfree = 0;
    g.scale = host_scale;
    g.dev_scale = dev_scale;
    return PRE_OK;
}

bool has_t(const Star &s) { return s.tm != 0.f || s.tp != 0.f; }

}  // namespace
