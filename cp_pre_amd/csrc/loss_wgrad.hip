// libcp_pre_wgrad.so (include/cp_pre_wgrad.h): the gradient of a residual loss with respect to a trainable operator kernel,
//   dk[dt][dx][dy] = scale * sum_c m_c * g_c * z_{c + (dt-1, dx-1, dy-1)},   z = x - y (y may be absent),
// in ONE streaming pass with a deterministic two-stage reduction (gfx950 only).
//
// The march.  A workgroup of 256 threads owns a tile of the (X,Y) plane and a segment [t0,t1) of g's planes, and walks
// the z planes t0-1 .. t1 (those that exist) along T, the slowest stencil axis:
//     acc[dt][dx][dy] += g_{t-dt+1}[c] * z_t[c + (dx-1, dy-1)]       for the 4 cells c of the thread's quad.
//   * g needs no halo: a thread keeps its own quad of the planes t-1, t, t+1 in a register ring, masked on load by a
//     select (the crop, the segment's ownership, the tile's edge);
//   * each z plane - x minus y, subtracted on load - is staged in LDS ONCE, with one halo row and one halo cell per side
//     (two buffers: the next plane is fetched while this one is used, one barrier per plane);
//   * 27 (9, 3, 1) fp32 accumulators per thread, added to fp64 ones after WG_FLUSH_PLANES planes at the latest: an fp32
//     accumulator never takes more than L = 4 * WG_FLUSH_PLANES = 32 products between two flushes;
//   * instantiated on the extents: a kt = 1 or kx = 1 operator carries neither the ring, the halo nor the taps it lacks.
//
// The constants (tests/wgrad_helpers.py restates them; the tests take their seams and their error bound from here):
//     tile          Y <= 32: 32 rows x 32 columns (8 quads a row);  else 16 rows x 64 columns (16 quads a row)
//     flush         WG_FLUSH_PLANES = 8 planes  ->  L = 32 cells
//     t segments    tSeg = T, halved (rounding up) while B * tiles * ceil(T / tSeg) < WG_MIN_UNITS = 1024 and
//                   tSeg > WG_MIN_TSEG = 8;  a unit is one (sample, segment, tile)
//     grid          min(units, WG_MAX_BLOCKS = 2048) workgroups; workgroup i takes the units i, i + grid, ...
// All of it is a function of the shape alone, so the order of every addition is.
//
// The Nt-fastest view (unit stride on T) needs no kernel of its own: dk of the view is dk of the relabelled array [B,X,Y,T]
// with the extents permuted; the crop is symmetric, so the mask is the same; the final stage writes dk in the logical
// (dt,dx,dy) order.  The march takes any sB, sX, sY there, as it takes any sB, sT, sX of a Y-fastest view: the cropped view
// of the reference's scripts, field[:, 0, 1:-1, 1:-1, 1:-1].permute(0, 3, 1, 2), is read where it lies.
#include "common.h"
#include "host_checks.h"
#include "../../include/cp_pre_wgrad.h"

namespace {

constexpr int WG_THREADS = 256;
constexpr int WG_FLUSH_PLANES = 8;
constexpr int WG_MIN_UNITS = 1024;
constexpr int WG_MIN_TSEG = 8;
constexpr int WG_MAX_TAPS = 27;
constexpr int WG_MAX_BLOCKS = PRE_WGRAD_WORKSPACE / WG_MAX_TAPS;
constexpr int WG_NARROW_Y = 32;
enum { CROP_T = 1, CROP_X = 2, CROP_Y = 4 };

struct WArgs {
    const float *g, *x, *y;
    long long gB, gT, gX, xB, xT, xX, yB, yT, yX;      // element strides of the kernel's axes (unit stride on Y)
    int B, T, X, Y;
    int crop;
    int tSeg, nSeg, tilesR, tilesC;
    long long units;
    double *partial;                                   // [grid][taps]
};

struct WMap {
    int idx[WG_MAX_TAPS];                              // tap of the march -> index in the logical dk
};

// (4-byte aligned float4 accesses: gfx950 runs with unaligned access enabled and the compiler still emits one
// global_load_dwordx4, so pitched and offset rows stream through the same code - as star_march.h)
struct __attribute__((aligned(4))) F4u { float x, y, z, w; };

// the cells col .. col+3 of a row of Y cells; only the elements lo <= j < hi, and only those inside the row, are read
__device__ __forceinline__ float4 ld_quad(const float *p, int col, int Y, int lo, int hi)
{
    if (lo == 0 && hi == 4 && col >= 0 && col + 3 < Y) {
        const F4u v = *reinterpret_cast<const F4u *>(p + col);
        return make_float4(v.x, v.y, v.z, v.w);
    }
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lo <= 0 && 0 < hi && col >= 0 && col < Y) v.x = p[col];
    if (lo <= 1 && 1 < hi && col + 1 >= 0 && col + 1 < Y) v.y = p[col + 1];
    if (lo <= 2 && 2 < hi && col + 2 >= 0 && col + 2 < Y) v.z = p[col + 2];
    if (lo <= 3 && 3 < hi && col + 3 >= 0 && col + 3 < Y) v.w = p[col + 3];
    return v;
}

template <int KT, int KX, int KY, int QPR>
__global__ void __launch_bounds__(WG_THREADS) wgrad_march_kernel(const WArgs a)
{
    constexpr int ROWS = WG_THREADS / QPR, COLS = 4 * QPR;
    constexpr int HT = KT == 3, HR = KX == 3, HC = KY == 3;
    constexpr int LR = ROWS + 2 * HR, LQ = QPR + 2 * HC, PITCH = 4 * LQ + 4;
    constexpr int NSLOT = LR * LQ, SPT = (NSLOT + WG_THREADS - 1) / WG_THREADS;
    constexpr int NT = KT * KX * KY;
    __shared__ __attribute__((aligned(16))) float zs[2][LR * PITCH];
    __shared__ double red[WG_THREADS / 64][NT];

    const int tid = threadIdx.x;
    const int q = tid % QPR, r = tid / QPR;
    const bool cT = a.crop & CROP_T, cX = a.crop & CROP_X, cY = a.crop & CROP_Y;

    float acc[KT][KX][KY];
    double dacc[KT][KX][KY];
#pragma unroll
    for (int i = 0; i < KT; ++i)
#pragma unroll
        for (int j = 0; j < KX; ++j)
#pragma unroll
            for (int k = 0; k < KY; ++k) { acc[i][j][k] = 0.f; dacc[i][j][k] = 0.0; }

    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        const int tc = (int)(u % a.tilesC);
        long long rest = u / a.tilesC;
        const int tr = (int)(rest % a.tilesR);
        rest /= a.tilesR;
        const int seg = (int)(rest % a.nSeg);
        const long long b = rest / a.nSeg;
        const int r0 = tr * ROWS, c0 = tc * COLS;
        const int t0 = seg * a.tSeg, t1 = min(t0 + a.tSeg, a.T);
        const int zlo = max(t0 - HT, 0), zhi = min(t1 + HT, a.T);
        const int row = r0 + r, col = c0 + 4 * q;

        // the thread's quad of g plane t: 0 unless the segment owns the plane and the loss averages over the cell
        const bool g_row = row < a.X && col < a.Y && !(cX && (row < 1 || row > a.X - 2));
        const float *gp0 = a.g + b * a.gB + (long long)row * a.gX;
        auto G = [&](int t) -> float4 {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!g_row || t < t0 || t >= t1 || (cT && (t < 1 || t > a.T - 2))) return v;
            v = ld_quad(gp0 + (long long)t * a.gT, col, a.Y, 0, 4);
            if (cY) {                                            // (a select: a non-finite g in the rim is not multiplied)
                if (col < 1 || col > a.Y - 2) v.x = 0.f;
                if (col + 1 > a.Y - 2) v.y = 0.f;
                if (col + 2 > a.Y - 2) v.z = 0.f;
                if (col + 3 > a.Y - 2) v.w = 0.f;
            }
            return v;
        };
        // the thread's share of z plane t (with its halo): x - y where the plane has cells, else 0
        float4 pre[SPT];
        auto fetch = [&](int t) {
#pragma unroll
            for (int k = 0; k < SPT; ++k) {
                const int s = tid + k * WG_THREADS;
                pre[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (s < NSLOT) {
                    const int lr = s / LQ, lq = s % LQ;
                    const int zr = r0 + lr - HR, zc = c0 + 4 * (lq - HC);
                    const int lo = (HC && lq == 0) ? 3 : 0, hi = (HC && lq == LQ - 1) ? 1 : 4;
                    if (zr >= 0 && zr < a.X) {
                        float4 v = ld_quad(a.x + b * a.xB + (long long)t * a.xT + (long long)zr * a.xX, zc, a.Y, lo, hi);
                        if (a.y) {
                            const float4 w = ld_quad(a.y + b * a.yB + (long long)t * a.yT + (long long)zr * a.yX, zc, a.Y, lo, hi);
                            v.x -= w.x; v.y -= w.y; v.z -= w.z; v.w -= w.w;
                        }
                        pre[k] = v;
                    }
                }
            }
        };
        auto stage = [&](int buf) {
#pragma unroll
            for (int k = 0; k < SPT; ++k) {
                const int s = tid + k * WG_THREADS;
                if (s < NSLOT) *reinterpret_cast<float4 *>(&zs[buf][(s / LQ) * PITCH + 4 * (s % LQ)]) = pre[k];
            }
        };
        auto flush = [&]() {
#pragma unroll
            for (int i = 0; i < KT; ++i)
#pragma unroll
                for (int j = 0; j < KX; ++j)
#pragma unroll
                    for (int k = 0; k < KY; ++k) { dacc[i][j][k] += (double)acc[i][j][k]; acc[i][j][k] = 0.f; }
        };

        // (every thread has left the last plane of the unit before: its closing barrier)
        fetch(zlo);
        stage(0);
        __syncthreads();
        int cur = 0, run = 0;
        float4 gm = G(zlo - 1), gc = G(zlo), gn = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int tz = zlo; tz < zhi; ++tz) {
            const bool more = tz + 1 < zhi;                      // (uniform over the workgroup)
            if (more) fetch(tz + 1);
            gn = G(tz + 1);
            float zr[KX][4 + 2 * HC];
#pragma unroll
            for (int dx = 0; dx < KX; ++dx) {
                const int base = (r + dx) * PITCH + 4 * (q + HC);
                const float4 c = *reinterpret_cast<const float4 *>(&zs[cur][base]);
                zr[dx][HC] = c.x; zr[dx][HC + 1] = c.y; zr[dx][HC + 2] = c.z; zr[dx][HC + 3] = c.w;
                if constexpr (HC != 0) {
                    zr[dx][0] = zs[cur][base - 1];
                    zr[dx][5] = zs[cur][base + 4];
                }
            }
#pragma unroll
            for (int dt = 0; dt < KT; ++dt) {
                const float4 gg = KT == 1 ? gc : dt == 0 ? gn : dt == 1 ? gc : gm;     // g_{tz - dt + 1}
#pragma unroll
                for (int dx = 0; dx < KX; ++dx)
#pragma unroll
                    for (int dy = 0; dy < KY; ++dy) {
                        float s = acc[dt][dx][dy];
                        s = fmaf(gg.x, zr[dx][dy], s);
                        s = fmaf(gg.y, zr[dx][dy + 1], s);
                        s = fmaf(gg.z, zr[dx][dy + 2], s);
                        s = fmaf(gg.w, zr[dx][dy + 3], s);
                        acc[dt][dx][dy] = s;
                    }
            }
            if (++run == WG_FLUSH_PLANES) {
                flush();
                run = 0;
            }
            if (more) stage(cur ^ 1);
            __syncthreads();
            cur ^= 1;
            gm = gc;
            gc = gn;
        }
        if (run) flush();
    }

    // the workgroup's partial of every tap: lanes by a fixed shuffle tree, the four waves in order
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int i = 0; i < KT; ++i)
#pragma unroll
        for (int j = 0; j < KX; ++j)
#pragma unroll
            for (int k = 0; k < KY; ++k) {
                double v = dacc[i][j][k];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
                if (lane == 0) red[wv][(i * KX + j) * KY + k] = v;
            }
    __syncthreads();
    if (tid < NT) {
        double v = red[0][tid];
#pragma unroll
        for (int w = 1; w < WG_THREADS / 64; ++w) v += red[w][tid];
        a.partial[(long long)blockIdx.x * NT + tid] = v;
    }
}

// Stage 2: a workgroup per tap adds that tap's partials (each thread its strided share, in order; then a fixed tree),
// applies the scale in fp64 and rounds once
__global__ void __launch_bounds__(256) wgrad_final_kernel(const double *partial, int nblocks, int ntaps, float host_scale,
                                                          const float *dev_scale, const WMap map, float *dk)
{
    __shared__ double red[256];
    const int tid = threadIdx.x, tap = blockIdx.x;
    double acc = 0.0;
    for (int i = tid; i < nblocks; i += 256) acc += partial[(long long)i * ntaps + tap];
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const double scale = (double)host_scale * (dev_scale ? (double)*dev_scale : 1.0);
        dk[map.idx[tap]] = (float)(scale * red[0]);
    }
}

// ------------------------------------------------------------------ host side
bool y_fastest(const pre_field_t *f) { return f->sY == 1; }
bool nt_fastest(const pre_field_t *f) { return f->sT == 1; }

template <int QPR>
int launch_march(int kt, int kx, int ky, unsigned grid, hipStream_t st, const WArgs &a)
{
#define WG_CASE(A, Bx, C)                                                                                               \
    if (kt == A && kx == Bx && ky == C) {                                                                               \
        hipLaunchKernelGGL((wgrad_march_kernel<A, Bx, C, QPR>), dim3(grid), dim3(WG_THREADS), 0, st, a);                \
        PRE_LAUNCH_CHECK();                                                                                             \
        return PRE_OK;                                                                                                  \
    }
    WG_CASE(1, 1, 1) WG_CASE(1, 1, 3) WG_CASE(1, 3, 1) WG_CASE(1, 3, 3)
    WG_CASE(3, 1, 1) WG_CASE(3, 1, 3) WG_CASE(3, 3, 1) WG_CASE(3, 3, 3)
#undef WG_CASE
    return PRE_E_UNSUPPORTED;
}

}  // namespace

extern "C" {

int pre_wgrad_abi_version(void) { return PRE_WGRAD_ABI_VERSION; }

int pre_wgrad_stencil3d_f32(const pre_field_t *g, const pre_field_t *x, const pre_field_t *y, int kt, int kx, int ky,
                            float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                            double *workspace, float *dk, void *stream)
{
    if (!g || !g->ptr || !x || !x->ptr || (y && !y->ptr) || !workspace || !dk) return PRE_E_NULL;
    if (B <= 0 || T <= 0 || X <= 0 || Y <= 0) return PRE_E_NULL;
    // (int32 cell indices, with room for the last tile's overhang)
    if (B > 0x7fffffff || T > 0x7fffffff - 128 || X > 0x7fffffff - 128 || Y > 0x7fffffff - 128) return PRE_E_SHAPE;
    const int ext[3] = {kt, kx, ky};
    for (int i = 0; i < 3; ++i)
        if (ext[i] != 1 && ext[i] != 3) return PRE_E_UNSUPPORTED;
    if (flags & ~(PRE_VJP_CROP | PRE_VJP_VIEW3D)) return PRE_E_UNSUPPORTED;
    if ((flags & PRE_VJP_VIEW3D) && kt != 1) return PRE_E_UNSUPPORTED;
    const pre_field_t *fs[3] = {g, x, y};
    const int nf = y ? 3 : 2;
    bool yfast = true, tfast = true;
    for (int i = 0; i < nf; ++i) {
        yfast = yfast && y_fastest(fs[i]);
        tfast = tfast && nt_fastest(fs[i]);
    }
    if (!yfast && !tfast) return PRE_E_UNSUPPORTED;
    // dk and the workspace are written: neither may lie on an input, nor on the other
    const int ntaps = kt * kx * ky;
    const Span sk{(uintptr_t)dk, (uintptr_t)dk + 4u * (uintptr_t)ntaps};
    const Span sw{(uintptr_t)workspace, (uintptr_t)workspace + 8u * (uintptr_t)PRE_WGRAD_WORKSPACE};
    if (overlaps(sk, sw)) return PRE_E_SHAPE;
    const int64_t n[4] = {B, T, X, Y};
    for (int i = 0; i < nf; ++i) {
        const int64_t s[4] = {fs[i]->sB, fs[i]->sT, fs[i]->sX, fs[i]->sY};
        Span f;
        if (!span_of(fs[i]->ptr, s, n, 0, &f) || overlaps(sk, f) || overlaps(sw, f)) return PRE_E_SHAPE;
    }

    // the kernel's axes: (T,X,Y) as given, or - Nt-fastest - the relabelled array [B,X,Y,T] with the extents permuted
    WArgs a;
    WMap map;
    int crop = 0;
    if (flags & PRE_VJP_CROP) crop = (flags & PRE_VJP_VIEW3D) ? (CROP_X | CROP_Y) : (CROP_T | CROP_X | CROP_Y);
    int k3[3];                                          // extents along the kernel's axes
    a.g = g->ptr; a.x = x->ptr; a.y = y ? y->ptr : nullptr;
    a.gB = g->sB; a.xB = x->sB; a.yB = y ? y->sB : 0;
    if (yfast) {
        a.T = (int)T; a.X = (int)X; a.Y = (int)Y;
        a.gT = g->sT; a.gX = g->sX; a.xT = x->sT; a.xX = x->sX; a.yT = y ? y->sT : 0; a.yX = y ? y->sX : 0;
        k3[0] = kt; k3[1] = kx; k3[2] = ky;
        a.crop = crop;
        for (int i = 0; i < ntaps; ++i) map.idx[i] = i;
    } else {
        a.T = (int)X; a.X = (int)Y; a.Y = (int)T;
        a.gT = g->sX; a.gX = g->sY; a.xT = x->sX; a.xX = x->sY; a.yT = y ? y->sX : 0; a.yX = y ? y->sY : 0;
        k3[0] = kx; k3[1] = ky; k3[2] = kt;
        a.crop = ((crop & CROP_X) ? CROP_T : 0) | ((crop & CROP_Y) ? CROP_X : 0) | ((crop & CROP_T) ? CROP_Y : 0);
        for (int i0 = 0; i0 < kx; ++i0)                 // march tap (dx, dy, dt) -> logical (dt, dx, dy)
            for (int i1 = 0; i1 < ky; ++i1)
                for (int i2 = 0; i2 < kt; ++i2) map.idx[(i0 * ky + i1) * kt + i2] = (i2 * kx + i0) * ky + i1;
    }
    for (int i = ntaps; i < WG_MAX_TAPS; ++i) map.idx[i] = 0;
    a.B = (int)B;

    // tile, t segments and grid: functions of the shape alone
    const bool narrow = a.Y <= WG_NARROW_Y;
    const int rows = narrow ? 32 : 16, cols = narrow ? 32 : 64;
    a.tilesR = (a.X + rows - 1) / rows;
    a.tilesC = (a.Y + cols - 1) / cols;
    const long long tiles = (long long)a.tilesR * a.tilesC;
    int tSeg = a.T;
    while ((long long)a.B * tiles * ((a.T + tSeg - 1) / tSeg) < WG_MIN_UNITS && tSeg > WG_MIN_TSEG) tSeg = (tSeg + 1) / 2;
    a.tSeg = tSeg;
    a.nSeg = (a.T + tSeg - 1) / tSeg;
    a.units = (long long)a.B * tiles * a.nSeg;
    const unsigned grid = (unsigned)(a.units < WG_MAX_BLOCKS ? a.units : WG_MAX_BLOCKS);
    a.partial = workspace;

    hipStream_t st = as_stream(stream);
    const int rc = narrow ? launch_march<8>(k3[0], k3[1], k3[2], grid, st, a) : launch_march<16>(k3[0], k3[1], k3[2], grid, st, a);
    if (rc) return rc;
    hipLaunchKernelGGL(wgrad_final_kernel, dim3((unsigned)ntaps), dim3(256), 0, st, workspace, (int)grid, ntaps, host_scale,
                       dev_scale, map, dk);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}

}  // extern "C"
