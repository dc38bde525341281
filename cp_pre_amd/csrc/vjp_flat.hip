// vjp_flat.hip - the vector-Jacobian products of residual_vjp.hip for Nt-fastest views of the 2-D residuals
// (libcp_pre_vjpflat.so, include/cp_pre_vjpflat.h): the backward pass of a physics-informed loss on fields whose memory is
// [B,Nx,Ny,Nt] - the view the reference's training scripts pass (Physics_Informed/Wave_FNO_PISL.py:209-217).
//
// The march templates are star_march.h's (Star, Nbr, apply<>, the LDS-only barrier, the buffer descriptors, flat_split),
// the functors vjp_functors.h's.  The march below is flat_march_kernel's (screen_flat.hip's) up to the functor: the kernel
// axes are relabelled as star_march.h's prepare() relabels them for an Nt-fastest view (marched axis = Nx, x = Ny, y = Nt), Ny and Nt are
// merged into one row of L = Ny*Nt cells, a workgroup owns a chunk of that row of ONE sample and marches a segment of Nx
// with planes t-1, t, t+1 and the in-flight t+2 of its own quads in registers.  x-neighbours are Nt cells back / ahead in
// the merged row, through LDS with a halo of ceil(Nt/4) quads per side; y-neighbours are the adjacent cell of the same LDS
// image; both are masked at row ends per element, because a quad straddles a row end when Nt % 4 != 0.
//
// What differs from the forward march is what vjp_march_kernel (residual_vjp.hip) does in the tiled form: stream 0 is the
// incoming gradient g, and what enters registers and LDS is gg = m ? scale * g : 0 - a select per LOGICAL cell (a merged-row
// position is (y, t) = (pos / Nt, pos % Nt), recovered per element, for the own quad and for the halo quad), so a NaN outside
// the crop reaches nothing; scale = host_scale * *dev_scale, the device scalar never read on the host.  Every stream is
// staged: the functors are general 7-point stars (mirrored and folded on the host in double, as residual_vjp.hip folds
// them, then relabelled to the kernel's axes), and the products gg*u, gg*v need the x-neighbours of u and v too.  Padding is
// zero (the adjoint of a zero-padded correlation).  Up to VF_MAXOUT (here three) output streams in the same merged order; marched planes
// are not cut by the crop: a rim plane's gradient is generally non-zero.  No atomics.
//
// The split (tests/vjpflat_helpers.py states it again and names the test seams from it):
//   chunk   flat_chunk(): 512 quads of the merged row per workgroup, or 448 ... 256 when that saves FLAT_NT_GAIN per cent
//           of chunks x (chunk + staged halo quads); the staged halo is 2 * min(32, ceil(Nt/4)) quads;
//   march   pick_tseg(B * chunks, Nx, resident workgroups): the marched axis in segments of tSeg planes.
#include "vjp_functors.h"
#include "../../include/cp_pre_vjpflat.h"

// 0: the NS-momentum instantiation is not built and its entry returns PRE_E_UNSUPPORTED (the project's rule for an
// instantiation that needs scratch inside the plane loop; csrc/resources.sh vjp_flat.hip is the check)
#ifndef PRE_VJPFLAT_NS
#define PRE_VJPFLAT_NS 1
#endif

// the streams a launch can take; a unit that includes this one with more of them (vjp_flat_mhd.hip) sets its own
#ifndef VF_MAXIN
#define VF_MAXIN 3
#endif
#ifndef VF_MAXOUT
#define VF_MAXOUT 3
#endif

namespace {

// Kernel axes: T = the marched axis (logical Nx), X = logical Ny, Y = logical Nt; a plane is one row of X * Y cells.
struct FVGeom {
    const float *f[VF_MAXIN];
    long long sB[VF_MAXIN], sT[VF_MAXIN];      // sample and marched-plane strides (elements)
    float *o[VF_MAXOUT];
    long long oB[VF_MAXOUT], oT[VF_MAXOUT];
    int B, T, X, Y;
    int tSeg, nTSeg, nCh;
    int crop;                    // cells per side the loss does not average over, on every axis (0 or 1)
    float scale;                 // host factor of g ...
    const float *dev_scale;      // ... times this device scalar, if given (the upstream gradient of loss.backward())
};

// ------------------------------------------------------------------ the march
template <class Fn>
__global__ void __launch_bounds__(FLAT_NT) vjp_flat_kernel(const FVGeom g, const typename Fn::Params prm)
{
    constexpr int F = Fn::FIN, FO = Fn::FOUT;
    __shared__ float4 lds[2][F][FLAT_NT + 2 * FLAT_H];
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

    // halo duty: the first / last HQ threads fetch one quad left / right of the chunk, HQ = the quads an x-neighbour (Ty
    // cells away) can reach into.  The LDS image keeps room for FLAT_H quads per side.
    const int HQ = min(FLAT_H, (Ty + 3) >> 2);
    const bool hl = q < HQ, hr = q >= NT - HQ;
    const int hm = hl ? m0 - 4 * (HQ - q) : m0 + 4 * NT + 4 * (q - (NT - HQ));
    const bool hok = (hl || hr) && hm >= 0 && hm < L;
    const int hslot = hl ? FLAT_H - HQ + q : FLAT_H + NT + (q - (NT - HQ));

    // per cell of my quad: does it have a y- / y+ neighbour inside its own x row, and does the loss average over it (bit j
    // of kown; khal: the same for my halo quad) - (x, y) = (pos / Ty, pos % Ty) recovered per element, because a quad
    // straddles a row end when Ty % 4 != 0
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
    // gg = m ? scale * g : 0, a select: whatever a masked cell holds stays where it is
    auto masked = [&](const float4 &v, unsigned k, bool kt) __attribute__((always_inline)) {
        return make_float4((kt && (k & 1u)) ? scale * v.x : 0.f, (kt && (k & 2u)) ? scale * v.y : 0.f,
                           (kt && (k & 4u)) ? scale * v.z : 0.f, (kt && (k & 8u)) ? scale * v.w : 0.f);
    };

    // a plane of a stream of this sample = a wave-uniform buffer descriptor; the thread's own quad and its halo quad are
    // two 32-bit byte offsets shared by every stream (one in-plane layout)
    const unsigned int voff = (unsigned int)m * 4u, hoff = (unsigned int)hm * 4u;       // (hm < 0: never loaded)
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    auto quad = [&](int i, int t, unsigned int off) __attribute__((always_inline)) {
        const float *p = g.f[i] + ((long long)b * g.sB[i] + (long long)t * g.sT[i]);
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(__builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, -1, 0x00020000),
                                                              (int)off, 0, 0);
        return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
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

    long long oo[FO];
#pragma unroll
    for (int k = 0; k < FO; ++k) oo[k] = (long long)b * g.oB[k] + m;

    // One plane.  P, C, N hold planes t-1, t, t+1 of the own quads, D receives plane t+2; hc is the halo quad of plane t, hn
    // receives that of plane t+1.  The caller rotates the roles instead of moving registers.
    auto step = [&](int t, float4(&P)[F], float4(&C)[F], float4(&N)[F], float4(&D)[F], float4(&hc)[F], float4(&hn)[F])
                    __attribute__((always_inline)) {
        const int bi = (t - t0) & 1;
#pragma unroll
        for (int i = 0; i < F; ++i) {
            lds[bi][i][FLAT_H + q] = C[i];
            if (hl || hr) lds[bi][i][hslot] = hc[i];
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
            const float *row = reinterpret_cast<const float *>(&lds[bi][i][0]) + 4 * (FLAT_H + q);      // my first cell
            if ((Ty & 1) == 0) {                     // Ty = 10, 30, 50 (T_out of the reference scripts): 8-byte aligned pairs
                const float2 a = *reinterpret_cast<const float2 *>(row - Ty), b2 = *reinterpret_cast<const float2 *>(row + 2 - Ty);
                const float2 c = *reinterpret_cast<const float2 *>(row + Ty), d = *reinterpret_cast<const float2 *>(row + 2 + Ty);
                n[i].xm = make_float4(a.x, a.y, b2.x, b2.y);
                n[i].xp = make_float4(c.x, c.y, d.x, d.y);
            } else {
                n[i].xm = make_float4(row[-Ty], row[1 - Ty], row[2 - Ty], row[3 - Ty]);
                n[i].xp = make_float4(row[Ty], row[Ty + 1], row[Ty + 2], row[Ty + 3]);
            }
            const float lft = row[-1], rgt = row[4];
            n[i].ym = make_float4(lok[0] ? lft : 0.f, lok[1] ? C[i].x : 0.f, lok[2] ? C[i].y : 0.f, lok[3] ? C[i].z : 0.f);
            n[i].yp = make_float4(rok[0] ? C[i].y : 0.f, rok[1] ? C[i].z : 0.f, rok[2] ? C[i].w : 0.f, rok[3] ? rgt : 0.f);
        }
        float4 r[FO];
        Fn::eval(n, prm, r);
        if (inb) {
#pragma unroll
            for (int k = 0; k < FO; ++k) stg4(g.o[k] + oo[k] + (long long)t * g.oT[k], r[k]);
        }
    };

    float4 w0[F], w1[F], w2[F], w3[F], h0[F], h1[F];
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
// prepare()'s relabelling of the star weights for kernel axes (X, Y, T): the logical x-taps sit on the marched axis, the
// y-taps on the kernel's x, the t-taps on its y
Star relabelled(const Star &o) { return Star{o.c, o.xm, o.xp, o.ym, o.yp, o.tm, o.tp}; }

template <class Fn>
int launch_vjp_flat(FVGeom &g, const typename Fn::Params &prm, hipStream_t st)
{
    static_assert(2 * Fn::FIN * (FLAT_NT + 2 * FLAT_H) * 16 <= 160 * 1024, "chunk does not fit the 160 KiB LDS");
    static_assert(FLAT_MAX_Y <= 4 * FLAT_H, "an x-neighbour must lie inside the staged halo");
    const long long quads = (long long)g.X * g.Y / 4;
    const int nt = flat_chunk(quads, g.Y, true);                   // (every stream is staged)
    g.nCh = (int)((quads + nt - 1) / nt);
    static std::atomic<int> per_cu[FLAT_NT / 64 + 1] = {};         // (by chunk width)
    unsigned grid;
    const int rc = flat_split(vjp_flat_kernel<Fn>, nt, per_cu, g, (long long)g.B * g.nCh, g.T, &grid);
    if (rc) return rc;
    hipLaunchKernelGGL((vjp_flat_kernel<Fn>), dim3(grid), dim3(nt), 0, st, g, prm);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}

// Null / empty / layout / overlap checks of everything an entry point hands to the kernel (residual_vjp.hip's prepare_vjp
// with the flat form's layout), every view against every other: an entry of several launches checks the views of all of
// them here before the first.  Shapes come in on the caller's logical [B,T,X,Y].
int check_vjp_flat(const pre_field_t *const *fs, int nf, const pre_out_t *const *os, int no, int64_t B, int64_t T, int64_t X,
                   int64_t Y, int flags)
{
    if (!vjp_views_given(fs, nf, os, no, B, T, X, Y)) return PRE_E_NULL;
    if (B > 0x7fffffff || T > 0x7fffffff || X > 0x7fffffff || Y > 0x7fffffff) return PRE_E_SHAPE;
    if (flags & ~PRE_VJP_CROP) return PRE_E_UNSUPPORTED;
    // the flat form's layout: T contiguous and short, dense rows, whole quads
    if (T >= FLAT_MAX_Y || (Y * T) % 4 != 0) return PRE_E_UNSUPPORTED;
    for (int i = 0; i < nf; ++i)
        if (fs[i]->sT != 1 || fs[i]->sY != T || fs[i]->sX != Y * T) return PRE_E_UNSUPPORTED;
    for (int k = 0; k < no; ++k)
        if (os[k]->sT != 1 || os[k]->sY != T || os[k]->sX != Y * T) return PRE_E_UNSUPPORTED;
    if (Y * T >= (1LL << 30)) return PRE_E_SHAPE;                  // a thread's place in a plane is a 32-bit byte offset
    if (!vjp_views_disjoint(fs, nf, os, no, B, T, X, Y)) return PRE_E_SHAPE;
    return PRE_OK;
}

// The checks above for the views of ONE launch, and its geometry on the kernel's axes.
int prepare_vjp_flat(FVGeom &g, const pre_field_t *const *fs, int nf, const pre_out_t *const *os, int no, int64_t B, int64_t T,
                     int64_t X, int64_t Y, int flags, float host_scale, const float *dev_scale)
{
    const int rc = check_vjp_flat(fs, nf, os, no, B, T, X, Y, flags);
    if (rc) return rc;
    for (int i = 0; i < VF_MAXIN; ++i) {
        const bool on = i < nf;
        g.f[i] = on ? fs[i]->ptr : nullptr;
        g.sB[i] = on ? fs[i]->sB : 0; g.sT[i] = on ? fs[i]->sX : 0;
    }
    for (int k = 0; k < VF_MAXOUT; ++k) {
        const bool on = k < no;
        g.o[k] = on ? os[k]->ptr : nullptr;
        g.oB[k] = on ? os[k]->sB : 0; g.oT[k] = on ? os[k]->sX : 0;
    }
    g.B = (int)B; g.T = (int)X; g.X = (int)Y; g.Y = (int)T;
    g.crop = (flags & PRE_VJP_CROP) ? 1 : 0;
    g.scale = host_scale;
    g.dev_scale = dev_scale;
    return PRE_OK;
}

}  // namespace

#ifndef PRE_VJPFLAT_NO_ENTRIES      // (vjp_flat_mhd.hip includes this unit for the march and its host side, not for the entries)
extern "C" {

int pre_vjpflat_abi_version(void) { return PRE_VJPFLAT_ABI_VERSION; }

int pre_vjpflat_stencil3d_f32(const pre_field_t *g, const pre_out_t *out, const float *tap_w, const int32_t *tap_off, int ntaps,
                              float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                              void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    const pre_field_t *fs[1] = {g};
    const pre_out_t *os[1] = {out};
    FVGeom vg;
    int rc = prepare_vjp_flat(vg, fs, 1, os, 1, B, T, X, Y, flags, host_scale, dev_scale);
    if (rc) return rc;
    Star s;
    if (!star_of_taps(tap_w, tap_off, ntaps, &s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    VjpLinear1::Params p{relabelled(mirrored(s))};
    return launch_vjp_flat<VjpLinear1>(vg, p, as_stream(stream));
}

int pre_vjpflat_linear2_f32(const pre_field_t *g, const pre_out_t out[2], const float *K_a, const float *K_b, float ratio,
                            float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                            void *stream)
{
    if (!out || !K_a || !K_b) return PRE_E_NULL;
    const pre_field_t *fs[1] = {g};
    const pre_out_t *os[2] = {&out[0], &out[1]};
    FVGeom vg;
    int rc = prepare_vjp_flat(vg, fs, 1, os, 2, B, T, X, Y, flags, host_scale, dev_scale);
    if (rc) return rc;
    Star a, b;
    if (!star_from_dense27(K_a, &a) || !star_from_dense27(K_b, &b)) return PRE_E_UNSUPPORTED;
    const Star zero{0, 0, 0, 0, 0, 0, 0};
    VjpLinear2::Params p{relabelled(mirrored(a)), relabelled(combine((double)ratio, mirrored(b), 0.0, zero))};
    return launch_vjp_flat<VjpLinear2>(vg, p, as_stream(stream));
}

int pre_vjpflat_ns_momentum_f32(const pre_field_t *g, const pre_field_t uv[2], const pre_out_t out[3], const float *K_t,
                                const float *K_x, const float *K_y, const float *K_xx_yy, float dt, float dx, float dy, float nu,
                                float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                void *stream)
{
    if (!uv || !out || !K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    const pre_field_t *fs[3] = {g, &uv[0], &uv[1]};
    const pre_out_t *os[3] = {&out[0], &out[1], &out[2]};
    FVGeom vg;
    int rc = prepare_vjp_flat(vg, fs, 3, os, 3, B, T, X, Y, flags, host_scale, dev_scale);
    if (rc) return rc;
    Star Dt, Dx, Dy, L;
    if (!star_from_dense27(K_t, &Dt) || !star_from_dense27(K_x, &Dx) || !star_from_dense27(K_y, &Dy) ||
        !star_from_dense27(K_xx_yy, &L))
        return PRE_E_UNSUPPORTED;
#if PRE_VJPFLAT_NS
    const double a = (double)dx * dy, b = (double)dt * dy, c = (double)dt * dx, n = (double)nu * dt;
    VjpNSMomentum::Params p;
    p.lin = relabelled(combine(a, mirrored(Dt), -n, mirrored(L)));
    p.pT = relabelled(combine(b, mirrored(Dx), c, mirrored(Dy)));
    p.Dx = relabelled(Dx); p.Dy = relabelled(Dy);
    p.DxT = relabelled(mirrored(Dx)); p.DyT = relabelled(mirrored(Dy));
    p.b = (float)b; p.c = (float)c;
    return launch_vjp_flat<VjpNSMomentum>(vg, p, as_stream(stream));
#else
    (void)dt; (void)dx; (void)dy; (void)nu; (void)stream;
    return PRE_E_UNSUPPORTED;      // the instantiation needs scratch: not built (csrc/resources.sh vjp_flat.hip)
#endif
}

}  // extern "C"
#endif
