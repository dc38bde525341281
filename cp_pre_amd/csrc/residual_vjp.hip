// residual_vjp.hip - vector-Jacobian products of the PDE residuals and the deterministic sum of squares of a residual
// (libcp_pre_vjp.so, include/cp_pre_vjp.h): what a physics-informed loss mean(r^2) needs for its backward pass.
//
// The march templates are star_march.h's (Star, Nbr, apply<>, the lane shifts, the LDS-only barrier, pick_tseg).
// The march of that header has ONE output stream and reads its inputs as stored; the gradient of NS momentum has THREE outputs, and the
// incoming gradient g has to be masked (the loss averages over the cropped interior) and scaled on load.  Hence a march of
// its own here, same structure: a workgroup of NR x TYQ threads owns NR rows x 4*TYQ columns of one sample and marches over
// t; every thread keeps planes t-1, t, t+1 (and the in-flight t+2) of its own quad per input stream in registers; the
// current plane goes through LDS (double-buffered, one barrier per plane) for the x-neighbours, halo rows included; the
// y-neighbours come from the adjacent lane, the two edge lanes of a row fetch one scalar.  Stream 0 is always g: what is
// kept in registers and LDS is gg = m ? scale * g : 0 (a select: a NaN outside the crop does not spread), so no masked or
// scaled copy of the residual ever exists in memory.  Widths that are no multiple of 4 are handled in the same launch: the
// last quad of a row loads and stores element by element.
//
// The functors of the linear operators and of NS momentum, with the folding of their stars, are vjp_functors.h's (shared
// with vjp_flat.hip); the Burgers functor has its only user here.
#include "vjp_functors.h"

namespace {

constexpr int VJP_MAXIN = 3, VJP_MAXOUT = 3;

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

// ------------------------------------------------------------------ the functor of Burgers: n[0] is gg, r[] the gradient
// r = dx*D_t(u) + dt*u*D_x(u) - nu*c3*D_xx(u):  du = (dx*D_t^T - nu*c3*D_xx^T)(gg) + dt*gg*D_x(u) + dt*D_x^T(gg*u)
struct VjpBurgers {
    static constexpr int FIN = 2, FOUT = 1;
    struct Params { Star lin, Dx, DxT; float dt; };      // lin = dx*Dt^T - nu*c3*Dxx^T
    static __device__ __forceinline__ void eval(const Nbr (&n)[2], const Params &p, float4 (&r)[1])
    {
        const Nbr gu = mul_nbr(n[0], n[1]);
        r[0] = apply<K_STAR7>(p.lin, n[0]) + p.dt * (mul4(n[0].c, apply<K_STAR7>(p.Dx, n[1])) + apply<K_STAR7>(p.DxT, gu));
    }
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
    static_assert(2 * Fn::FIN * (NR + 2) * TYQ * 16 <= 64 * 1024, "static LDS of a workgroup");
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

// ------------------------------------------------------------------ sum(m * r^2): two stages, fixed order, fp64
constexpr int SUMSQ_WAVES = 4;

// Stage 1: a wave per row of the [B*T*X, Y] view (rows dealt round-robin over the grid's waves), a lane per quad; every
// lane adds its squares in fp64 in the order it meets them, the workgroup's 256 lane sums are added by a fixed tree in LDS.
__global__ void __launch_bounds__(64 *SUMSQ_WAVES) sumsq_partial_kernel(const float *r, long long sB, long long sT, long long sX,
                                                                        int T, int X, int Y, long long rows, int crop,
                                                                        double *partial)
{
    __shared__ double red[64 * SUMSQ_WAVES];
    const int lane = threadIdx.x, wv = threadIdx.y;
    const bool cT = crop & CROP_T, cX = crop & CROP_X, cY = crop & CROP_Y;
    double acc = 0.0;
    for (long long row = (long long)blockIdx.x * SUMSQ_WAVES + wv; row < rows; row += (long long)gridDim.x * SUMSQ_WAVES) {
        const int x = (int)(row % X);
        const long long bt = row / X;
        const int t = (int)(bt % T);
        const long long b = bt / T;
        if ((cT && (t < 1 || t > T - 2)) || (cX && (x < 1 || x > X - 2))) continue;       // (wave-uniform)
        const float *p = r + b * sB + (long long)t * sT + (long long)x * sX;
        for (int y = 4 * lane; y < Y; y += 256) {
            float4 v = f4(0.f);
            if (y + 3 < Y) {
                v = ldg4(p + y);
            } else {
                v.x = p[y];
                if (y + 1 < Y) v.y = p[y + 1];
                if (y + 2 < Y) v.z = p[y + 2];
            }
            if (cY) {
                if (y < 1 || y > Y - 2) v.x = 0.f;                       // (a select: a NaN outside the crop is not summed)
                if (y + 1 > Y - 2) v.y = 0.f;
                if (y + 2 > Y - 2) v.z = 0.f;
                if (y + 3 > Y - 2) v.w = 0.f;
            }
            acc += ((double)v.x * (double)v.x + (double)v.y * (double)v.y) + ((double)v.z * (double)v.z + (double)v.w * (double)v.w);
        }
    }
    const int tid = wv * 64 + lane;
    red[tid] = acc;
    __syncthreads();
    for (int s = 32 * SUMSQ_WAVES; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = red[0];
}

// Stage 2: one workgroup adds the partials (each thread its strided share, in order; then the same fixed tree)
__global__ void __launch_bounds__(256) sumsq_final_kernel(const double *partial, int n, double *out)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n; i += 256) acc += partial[i];
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) *out = red[0];
}

}  // namespace

extern "C" {

int pre_vjp_abi_version(void) { return PRE_VJP_ABI_VERSION; }

int pre_vjp_stencil3d_f32(const pre_field_t *g, const pre_out_t *out, const float *tap_w, const int32_t *tap_off, int ntaps,
                          float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                          void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    const pre_field_t *fs[1] = {g};
    const pre_out_t *os[1] = {out};
    VGeom vg;
    int rc = prepare_vjp(vg, fs, 1, os, 1, B, T, X, Y, crop_of(flags, false), host_scale, dev_scale);
    if (rc) return rc;
    Star s;
    if (!star_of_taps(tap_w, tap_off, ntaps, &s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    VjpLinear1::Params p{mirrored(s)};
    vg.tfree = !has_t(s);
    return launch_vjp<VjpLinear1>(vg, p, as_stream(stream));
}

int pre_vjp_stencil2d_f32(const float *g, const int64_t g_strides[3], float *out, const int64_t out_strides[3],
                          const float *tap_w, const int32_t *tap_off, int ntaps, float host_scale, const float *dev_scale,
                          int64_t B, int64_t T, int64_t X, int flags, void *stream)
{
    if (!g || !g_strides || !out || !out_strides || ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    // [B,T,X] with taps (dt,dx)  ==  [1,B,T,X] with taps (0,dt,dx)
    int32_t off3[3 * 343];
    for (int i = 0; i < ntaps; ++i) {
        off3[3 * i] = 0;
        off3[3 * i + 1] = tap_off[2 * i];
        off3[3 * i + 2] = tap_off[2 * i + 1];
    }
    pre_field_t fg{g, 0, g_strides[0], g_strides[1], g_strides[2]};
    pre_out_t o{out, 0, out_strides[0], out_strides[1], out_strides[2]};
    const pre_field_t *fs[1] = {&fg};
    const pre_out_t *os[1] = {&o};
    VGeom vg;
    int rc = prepare_vjp(vg, fs, 1, os, 1, 1, B, T, X, crop_of(flags, true), host_scale, dev_scale);
    if (rc) return rc;
    Star s;
    if (!star_of_taps(tap_w, off3, ntaps, &s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    VjpLinear1::Params p{mirrored(s)};
    vg.tfree = 1;
    return launch_vjp<VjpLinear1>(vg, p, as_stream(stream));
}

int pre_vjp_linear2_f32(const pre_field_t *g, const pre_out_t out[2], const float *K_a, const float *K_b, float ratio,
                        float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                        void *stream)
{
    if (!out || !K_a || !K_b) return PRE_E_NULL;
    const pre_field_t *fs[1] = {g};
    const pre_out_t *os[2] = {&out[0], &out[1]};
    VGeom vg;
    int rc = prepare_vjp(vg, fs, 1, os, 2, B, T, X, Y, crop_of(flags, false), host_scale, dev_scale);
    if (rc) return rc;
    Star a, b;
    if (!star_from_dense27(K_a, &a) || !star_from_dense27(K_b, &b)) return PRE_E_UNSUPPORTED;
    const Star zero{0, 0, 0, 0, 0, 0, 0};
    VjpLinear2::Params p{mirrored(a), combine((double)ratio, mirrored(b), 0.0, zero)};
    vg.tfree = !has_t(a) && !has_t(b);
    return launch_vjp<VjpLinear2>(vg, p, as_stream(stream));
}

int pre_vjp_burgers_f32(const float *g, const int64_t g_strides[3], const float *u, const int64_t u_strides[3], float *du,
                        const int64_t du_strides[3], const float *K_t, const float *K_x, const float *K_xx, float dx, float dt,
                        float nu, float c3, float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X,
                        int flags, void *stream)
{
    if (!g || !g_strides || !u || !u_strides || !du || !du_strides || !K_t || !K_x || !K_xx) return PRE_E_NULL;
    // [B,T,X] -> [1,B,T,X]; 3x3 kernel (a over Nt, b over Nx) -> dense27 index (1, a, b), as pre_residual_burgers_f32
    pre_field_t fg{g, 0, g_strides[0], g_strides[1], g_strides[2]}, fu{u, 0, u_strides[0], u_strides[1], u_strides[2]};
    pre_out_t o{du, 0, du_strides[0], du_strides[1], du_strides[2]};
    const pre_field_t *fs[2] = {&fg, &fu};
    const pre_out_t *os[1] = {&o};
    VGeom vg;
    int rc = prepare_vjp(vg, fs, 2, os, 1, 1, B, T, X, crop_of(flags, true), host_scale, dev_scale);
    if (rc) return rc;
    float d27[3][27] = {};
    const float *k9[3] = {K_t, K_x, K_xx};
    for (int op = 0; op < 3; ++op)
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) d27[op][(1 * 3 + i) * 3 + c] = k9[op][i * 3 + c];
    Star Dt, Dx, Dxx;
    if (!star_from_dense27(d27[0], &Dt) || !star_from_dense27(d27[1], &Dx) || !star_from_dense27(d27[2], &Dxx))
        return PRE_E_UNSUPPORTED;
    VjpBurgers::Params p;
    p.lin = combine((double)dx, mirrored(Dt), -((double)nu * (double)c3), mirrored(Dxx));
    p.Dx = Dx;
    p.DxT = mirrored(Dx);
    p.dt = dt;
    vg.tfree = 1;
    return launch_vjp<VjpBurgers>(vg, p, as_stream(stream));
}

int pre_vjp_ns_momentum_f32(const pre_field_t *g, const pre_field_t uv[2], const pre_out_t out[3], const float *K_t,
                            const float *K_x, const float *K_y, const float *K_xx_yy, float dt, float dx, float dy, float nu,
                            float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                            void *stream)
{
    if (!uv || !out || !K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    const pre_field_t *fs[3] = {g, &uv[0], &uv[1]};
    const pre_out_t *os[3] = {&out[0], &out[1], &out[2]};
    VGeom vg;
    int rc = prepare_vjp(vg, fs, 3, os, 3, B, T, X, Y, crop_of(flags, false), host_scale, dev_scale);
    if (rc) return rc;
    Star Dt, Dx, Dy, L;
    if (!star_from_dense27(K_t, &Dt) || !star_from_dense27(K_x, &Dx) || !star_from_dense27(K_y, &Dy) ||
        !star_from_dense27(K_xx_yy, &L))
        return PRE_E_UNSUPPORTED;
    const double a = (double)dx * dy, b = (double)dt * dy, c = (double)dt * dx, n = (double)nu * dt;
    VjpNSMomentum::Params p;
    p.lin = combine(a, mirrored(Dt), -n, mirrored(L));
    p.pT = combine(b, mirrored(Dx), c, mirrored(Dy));
    p.Dx = Dx; p.Dy = Dy;
    p.DxT = mirrored(Dx); p.DyT = mirrored(Dy);
    p.b = (float)b; p.c = (float)c;
    vg.tfree = !has_t(Dt) && !has_t(Dx) && !has_t(Dy) && !has_t(L);
    return launch_vjp<VjpNSMomentum>(vg, p, as_stream(stream));
}

int pre_vjp_sumsq_f32(const pre_field_t *r, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, double *workspace,
                      double *out, void *stream)
{
    if (!r || !r->ptr || !workspace || !out || B <= 0 || T <= 0 || X <= 0 || Y <= 0) return PRE_E_NULL;
    if (B > 0x7fffffff || T > 0x7fffffff || X > 0x7fffffff || Y > 0x7fffffff - 8) return PRE_E_SHAPE;
    if (r->sY != 1) return PRE_E_UNSUPPORTED;
    const long long rows = (long long)B * T * X;
    // the grid is a function of the shape alone: the same view is always summed in the same order
    const long long want = (rows + SUMSQ_WAVES - 1) / SUMSQ_WAVES;
    const int blocks = (int)(want < PRE_VJP_SUMSQ_WORKSPACE ? want : PRE_VJP_SUMSQ_WORKSPACE);
    int crop = 0;
    if (flags & PRE_VJP_CROP) crop = (flags & PRE_VJP_VIEW3D) ? (CROP_X | CROP_Y) : (CROP_T | CROP_X | CROP_Y);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3((unsigned)blocks), dim3(64, SUMSQ_WAVES), 0, st, r->ptr, (long long)r->sB,
                       (long long)r->sT, (long long)r->sX, (int)T, (int)X, (int)Y, rows, crop, workspace);
    PRE_LAUNCH_CHECK();
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, st, workspace, blocks, out);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}

}  // extern "C"
