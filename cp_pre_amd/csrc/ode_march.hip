// ODE operators and fused ODE residuals on [BS, Nt] fields (include/cp_pre_ode.h): the reference's Utils/ConvOps_0d.py
// stencil (F.conv1d with padding k//2) and the residuals of its ODE scripts, sum_i c_i[t] * (K_i ⋆ x_i).
//
// Work split.  The BS x Nt outputs are taken in flat (b, t) order, t fastest, and each thread owns ODE_V consecutive ones,
// so short rows (Nt = 100) pack many rows into one wave and long rows (Nt = 4096+) spread over many waves; no lane idles
// on a row end.  A thread keeps one K-wide window per source field in registers and slides it: one new load per source
// and output, the full window reloaded only where its run starts or crosses into the next row.  The halo (at most 3
// values per side) is therefore read again only by the neighbouring thread, from cache.
//
// Sources.  The host groups terms by field view, so terms on the same view (Bessel: three terms on y) share one window.
// Terms on different components of one [BS, Nt, S] tensor are different views, but a thread loads all of them for the
// same (b, t) back to back: the interleaved cache lines are fetched from HBM once and the other components hit in cache.
//
// Wgrad.  A fixed grid of PRE_ODE_WGRAD_BLOCKS workgroups, each over a fixed flat range of (b, t); fp64 per-thread sums,
// a fixed-shape LDS tree, one partial per workgroup and tap, then one workgroup sums the partials in a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cp_pre_ode.h"
#include "../../include/cp_pre_hip.h"

namespace {

constexpr int ODE_BLOCK = 256;
constexpr int ODE_V = 4;            // consecutive outputs per thread
constexpr int WG_BLOCK = 256;

struct Src {
    const float *p;
    long long sB, sT;
};

struct Term {
    const float *c;
    int src;                        // index into OdeArgs::src
    int lo, hi;                     // the term's taps occupy window slots [lo, hi] of the K-wide window
    float w[PRE_ODE_MAX_TAPS];      // taps at their window slots (slot j <-> offset j - K/2)
};

struct OdeArgs {
    Src src[PRE_ODE_MAX_TERMS];
    Term term[PRE_ODE_MAX_TERMS];
    float *out;
    long long oB, oT;
    long long Nt, total;
    int nsrc, nterm, absval, narrow;   // narrow: total < 2^32, the flat index divides in 32 bits
};

template <int K>
__global__ void __launch_bounds__(ODE_BLOCK) ode_residual_kernel(const OdeArgs a)
{
    constexpr int H = K / 2;
    const long long start = ((long long)blockIdx.x * ODE_BLOCK + threadIdx.x) * ODE_V;
    if (start >= a.total) return;
    long long b, t;
    if (a.narrow) {
        const unsigned s = (unsigned)start, n = (unsigned)a.Nt;
        const unsigned q = s / n;
        b = q;
        t = s - q * n;
    } else {
        b = start / a.Nt;
        t = start - b * a.Nt;
    }
    const long long Nt = a.Nt;
    float win[PRE_ODE_MAX_TERMS][K];

#pragma unroll
    for (int v = 0; v < ODE_V; ++v) {
        if (start + v >= a.total) break;
        const bool fresh = (v == 0) || (t == 0);
#pragma unroll
        for (int s = 0; s < PRE_ODE_MAX_TERMS; ++s) {
            if (s >= a.nsrc) break;
            const float *row = a.src[s].p + b * a.src[s].sB;
            const long long sT = a.src[s].sT;
            if (fresh) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const long long u = t - H + j;
                    win[s][j] = (u >= 0 && u < Nt) ? row[u * sT] : 0.0f;
                }
            } else {
#pragma unroll
                for (int j = 0; j + 1 < K; ++j) win[s][j] = win[s][j + 1];
                const long long u = t + H;
                win[s][K - 1] = (u < Nt) ? row[u * sT] : 0.0f;
            }
        }
        float acc = 0.0f;
#pragma unroll
        for (int s = 0; s < PRE_ODE_MAX_TERMS; ++s) {
            if (s >= a.nsrc) break;
#pragma unroll
            for (int i = 0; i < PRE_ODE_MAX_TERMS; ++i) {
                if (i >= a.nterm) break;
                if (a.term[i].src != s) continue;
                float d = 0.0f;
#pragma unroll
                for (int j = 0; j < K; ++j)
                    if (j >= a.term[i].lo && j <= a.term[i].hi) d = fmaf(a.term[i].w[j], win[s][j], d);
                if (a.term[i].c) d = a.term[i].c[t] * d;
                acc += d;
            }
        }
        a.out[b * a.oB + t * a.oT] = a.absval ? fabsf(acc) : acc;
        if (++t == Nt) {
            t = 0;
            ++b;
        }
    }
}

struct WgArgs {
    const float *x;
    long long xB, xT;
    const float *g;
    long long gB, gT;
    long long Nt, total, per;          // per: flat elements per workgroup
    double *work;
};

template <int K>
__global__ void __launch_bounds__(WG_BLOCK) ode_wgrad_partial_kernel(const WgArgs a)
{
    constexpr int H = K / 2;
    __shared__ double red[K][WG_BLOCK];
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    const long long e0 = (long long)blockIdx.x * a.per;
    const long long e1 = min(e0 + a.per, a.total);
    for (long long e = e0 + threadIdx.x; e < e1; e += WG_BLOCK) {
        const long long b = e / a.Nt, t = e - b * a.Nt;
        const double gv = (double)a.g[b * a.gB + t * a.gT];
        const float *row = a.x + b * a.xB;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const long long u = t - H + j;
            const float xv = (u >= 0 && u < a.Nt) ? row[u * a.xT] : 0.0f;
            acc[j] = fma(gv, (double)xv, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) red[j][threadIdx.x] = acc[j];
    __syncthreads();
    for (int w = WG_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int j = 0; j < K; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < K) a.work[(long long)blockIdx.x * K + threadIdx.x] = red[threadIdx.x][0];
}

__global__ void __launch_bounds__(WG_BLOCK) ode_wgrad_final_kernel(const double *work, int k, float *dk)
{
    __shared__ double red[WG_BLOCK];
    for (int j = 0; j < k; ++j) {
        double s = 0.0;
        for (int p = threadIdx.x; p < PRE_ODE_WGRAD_BLOCKS; p += WG_BLOCK) s += work[(long long)p * k + j];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int w = WG_BLOCK / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) dk[j] = (float)red[0];
        __syncthreads();
    }
}

bool bad_k(int k) { return k < 1 || k > PRE_ODE_MAX_TAPS || (k % 2) == 0; }

// An output view of BS x Nt elements writes each address at most once: every axis longer than 1 has a non-zero stride,
// and the axis of larger |stride| steps over the whole extent of the other one.
bool self_overlapping(long long BS, long long Nt, long long sB, long long sT)
{
    const bool mb = BS > 1, mt = Nt > 1;
    if ((mb && sB == 0) || (mt && sT == 0)) return true;
    if (!(mb && mt)) return false;
    long long ab = sB < 0 ? -sB : sB, at = sT < 0 ? -sT : sT;
    if (ab >= at) return ab < Nt * at;
    return at < BS * ab;
}

int launch_residual(OdeArgs &a, int K, hipStream_t st)
{
    const long long per_block = (long long)ODE_BLOCK * ODE_V;
    const long long nb = (a.total + per_block - 1) / per_block;
    const dim3 grid((unsigned)nb), block(ODE_BLOCK);
    switch (K) {
    case 1: hipLaunchKernelGGL(ode_residual_kernel<1>, grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL(ode_residual_kernel<3>, grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL(ode_residual_kernel<5>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(ode_residual_kernel<7>, grid, block, 0, st, a); break;
    }
    return (int)hipGetLastError();
}

int residual_impl(const pre_ode_term_t *terms, int nterms, float *out, const int64_t *os, int64_t BS, int64_t Nt, int flags,
                  void *stream)
{
    if (!terms || !out || !os || BS < 0 || Nt < 0) return PRE_E_NULL;
    if (nterms < 1 || nterms > PRE_ODE_MAX_TERMS) return PRE_E_UNSUPPORTED;
    int K = 1;
    for (int i = 0; i < nterms; ++i) {
        if (bad_k(terms[i].k)) return PRE_E_UNSUPPORTED;
        if (!terms[i].x) return PRE_E_NULL;
        if (terms[i].k > K) K = terms[i].k;
    }
    if (self_overlapping(BS, Nt, os[0], os[1])) return PRE_E_SHAPE;
    if ((long long)BS > (1LL << 40) / (Nt > 0 ? Nt : 1)) return PRE_E_SHAPE;        // flat index and grid size stay in range
    if (BS == 0 || Nt == 0) return PRE_OK;
    OdeArgs a = {};
    const int H = K / 2;
    for (int i = 0; i < nterms; ++i) {
        const pre_ode_term_t &tm = terms[i];
        int s = 0;
        for (; s < a.nsrc; ++s)
            if (a.src[s].p == tm.x && a.src[s].sB == tm.sB && a.src[s].sT == tm.sT) break;
        if (s == a.nsrc) a.src[a.nsrc++] = Src{tm.x, tm.sB, tm.sT};
        Term &d = a.term[i];
        d.c = tm.c;
        d.src = s;
        d.lo = H - tm.k / 2;
        d.hi = H + tm.k / 2;
        for (int j = 0; j < tm.k; ++j) d.w[d.lo + j] = tm.taps[j];
    }
    a.nterm = nterms;
    a.out = out;
    a.oB = os[0];
    a.oT = os[1];
    a.Nt = Nt;
    a.total = BS * Nt;
    a.absval = (flags & PRE_ODE_FLAG_ABS) ? 1 : 0;
    a.narrow = a.total < (1LL << 32) ? 1 : 0;
    return launch_residual(a, K, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int pre_ode_abi_version(void) { return PRE_ODE_ABI_VERSION; }

int pre_ode_stencil_f32(const float *in, const int64_t in_strides[2], float *out, const int64_t out_strides[2], int64_t BS,
                        int64_t Nt, const float *taps, int k, int flags, void *stream)
{
    if (!in || !in_strides || !taps) return PRE_E_NULL;
    if (bad_k(k)) return PRE_E_UNSUPPORTED;
    pre_ode_term_t t = {};
    t.x = in;
    t.sB = in_strides[0];
    t.sT = in_strides[1];
    t.c = nullptr;
    t.k = k;
    for (int j = 0; j < k; ++j) t.taps[j] = taps[j];
    return residual_impl(&t, 1, out, out_strides, BS, Nt, flags, stream);
}

int pre_ode_residual_f32(const pre_ode_term_t *terms, int nterms, float *out, const int64_t out_strides[2], int64_t BS,
                         int64_t Nt, int flags, void *stream)
{
    return residual_impl(terms, nterms, out, out_strides, BS, Nt, flags, stream);
}

int pre_ode_wgrad_f32(const float *x, const int64_t x_strides[2], const float *g, const int64_t g_strides[2], int64_t BS,
                      int64_t Nt, int k, double *work, float *dk, void *stream)
{
    if (!x || !x_strides || !g || !g_strides || !work || !dk || BS < 0 || Nt < 0) return PRE_E_NULL;
    if (bad_k(k)) return PRE_E_UNSUPPORTED;
    if ((long long)BS > (1LL << 40) / (Nt > 0 ? Nt : 1)) return PRE_E_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    WgArgs a;
    a.x = x;
    a.xB = x_strides[0];
    a.xT = x_strides[1];
    a.g = g;
    a.gB = g_strides[0];
    a.gT = g_strides[1];
    a.Nt = Nt > 0 ? Nt : 1;
    a.total = BS * Nt;
    a.per = (a.total + PRE_ODE_WGRAD_BLOCKS - 1) / PRE_ODE_WGRAD_BLOCKS;
    a.work = work;
    const dim3 grid(PRE_ODE_WGRAD_BLOCKS), block(WG_BLOCK);
    // (an empty field still runs both passes: every partial is 0 and dk is written)
    switch (k) {
    case 1: hipLaunchKernelGGL(ode_wgrad_partial_kernel<1>, grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL(ode_wgrad_partial_kernel<3>, grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL(ode_wgrad_partial_kernel<5>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(ode_wgrad_partial_kernel<7>, grid, block, 0, st, a); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(ode_wgrad_final_kernel, dim3(1), block, 0, st, (const double *)work, k, dk);
    return (int)hipGetLastError();
}

}  // extern "C"
