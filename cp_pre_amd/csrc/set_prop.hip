// PRE set propagation (include/cp_pre_setprop.h): per row, two circulant products in fp64,
//     centre_k = sum_j c_j g[(k - j) mod N],  radius_k = sum_j r_j a[(k - j) mod N],
// which is the closed form of the reference's zonotope pipeline (Inverted_bounds/intervalFFT.py, SHO.py set_PRE).
//
// Work split.  A workgroup owns an output tile of TK columns k (one per thread) and RB rows; each thread accumulates
// SP_TB rows of its column in registers.  TK is 64, 128 or 256 by N, so short rows (the scripts' N = 101) pack 32 or 16
// rows into one workgroup instead of idling lanes past the row end.  The j axis is walked in chunks of SP_TJ: per chunk the
// workgroup stages the window of the tables that its columns meet (TK + SP_TJ - 1 entries, wrapped mod N) and the c / r
// values of its rows in LDS.  Lane k then reads table entry (k - j) and its neighbour lane (k + 1 - j): consecutive
// 64-bit words, no bank conflict; the row values at j are the same address for the whole wave (a broadcast), stored
// [j][row] so one lane's SP_TB rows are one contiguous 64-byte read.  Tables of any N are tiled this way; nothing scales
// LDS with N.
//
// Recipe.  The fused form reads field rows and builds the interval set as it stages a chunk: r_j = |conv[j + 1]| (or
// q-hat) for the interior, computed from at most 7 taps of the fp32 field in fp64 (the reference upcasts before its FFT).
// The centre has four non-zeros (conv[1..3], conv[Nt + 1]), so it is four FMAs per output outside the loop.
//
// Determinism.  Every sum runs j = 0, 1, ... in one fixed order; grid shape and summation order depend only on (B, N).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/cp_pre_setprop.h"
#include "../../include/cp_pre_hip.h"

namespace {

constexpr int SP_BLOCK = 256;
constexpr int SP_TB = 8;            // rows per thread
constexpr int SP_TJ = 32;           // j per staged chunk

enum { MODE_F32 = 0, MODE_F64 = 1, MODE_RECIPE = 2 };

struct SpArgs {
    const void *c, *r;              // bounds: row operands
    long long cB, cT, rB, rT;
    const float *f;                 // recipe: field rows, Nt = N - 1 steps
    long long fB, fT;
    const float *q;                 // recipe: q-hat or null
    long long qB, qT;
    double taps[PRE_SETPROP_MAX_TAPS];
    int k, corr, qshift;            // qshift: t = n + qshift
    const double *g, *a;
    double *lo, *hi;
    long long B, N;
    long long tiles;                // output tiles per row group
};

__device__ __forceinline__ long long wrap(long long m, long long n)
{
    m %= n;
    return m < 0 ? m + n : m;
}

// conv[n] of the padded field s = [0, field, 0] (length N + 1), n in [1, N]
__device__ __forceinline__ double recipe_conv(const SpArgs &a, const float *row, long long n)
{
    const long long Ns = a.N + 1, Nt = a.N - 1;
    double acc = 0.0;
    for (int i = 0; i < a.k; ++i) {
        const long long m = wrap(a.corr ? n + i : n - i, Ns);
        const double s = (m >= 1 && m <= Nt) ? (double)row[(m - 1) * a.fT] : 0.0;
        acc = fma(a.taps[i], s, acc);
    }
    return acc;
}

template <int TK, int MODE>
__global__ void __launch_bounds__(SP_BLOCK) setprop_kernel(const SpArgs a)
{
    constexpr int GROUPS = SP_BLOCK / TK;
    constexpr int RB = SP_TB * GROUPS;
    constexpr int W = TK + SP_TJ - 1;
    constexpr bool HAS_C = MODE != MODE_RECIPE;
    __shared__ double tg[HAS_C ? W : 1], ta[W];
    __shared__ double sc[HAS_C ? SP_TJ : 1][RB], sr[SP_TJ][RB];
    __shared__ double cedge[MODE == MODE_RECIPE ? RB : 1][4];
    __shared__ int bad[RB];

    const int tid = threadIdx.x;
    const int kk = tid % TK, grp = tid / TK;
    const long long tile = blockIdx.x % a.tiles, rg = blockIdx.x / a.tiles;
    const long long k0 = tile * TK, row0 = rg * RB;
    const long long N = a.N, B = a.B;
    const long long k = k0 + kk;

    if (tid < RB) bad[tid] = 0;
    if constexpr (MODE == MODE_RECIPE) if (tid < RB * 4) {
        const int row = tid / 4, e = tid % 4;
        const long long b = row0 + row;
        double v = 0.0;
        if (b < B) v = recipe_conv(a, a.f + b * a.fB, e < 3 ? e + 1 : N);
        cedge[row][e] = v;
    }
    __syncthreads();                                // bad[] is cleared before any chunk may set it

    double cen[SP_TB], rad[SP_TB];
#pragma unroll
    for (int i = 0; i < SP_TB; ++i) cen[i] = rad[i] = 0.0;

    for (long long j0 = 0; j0 < N; j0 += SP_TJ) {
        const long long base = k0 - j0 - (SP_TJ - 1);
        for (int w = tid; w < W; w += SP_BLOCK) {
            const long long m = wrap(base + w, N);
            ta[w] = a.a[m];
            if constexpr (HAS_C) tg[w] = a.g[m];
        }
        for (int e = tid; e < SP_TJ * RB; e += SP_BLOCK) {
            const int row = e / SP_TJ, jj = e % SP_TJ;
            const long long b = row0 + row, j = j0 + jj;
            double cv = 0.0, rv = 0.0;
            if (b < B && j < N) {
                if (MODE == MODE_F32) {
                    cv = ((const float *)a.c)[b * a.cB + j * a.cT];
                    rv = ((const float *)a.r)[b * a.rB + j * a.rT];
                } else if (MODE == MODE_F64) {
                    cv = ((const double *)a.c)[b * a.cB + j * a.cT];
                    rv = ((const double *)a.r)[b * a.rB + j * a.rT];
                } else {
                    const long long n = j + 1;
                    const double x = recipe_conv(a, a.f + b * a.fB, n);
                    if (!isfinite(x)) bad[row] = 1;
                    if (j >= 3 && j <= N - 2) {
                        const long long t = n + a.qshift;
                        rv = (a.q && t >= 0 && t < N - 1) ? (double)a.q[b * a.qB + t * a.qT] : fabs(x);
                    }
                }
            }
            if constexpr (HAS_C) sc[jj][row] = cv;
            sr[jj][row] = rv;
        }
        __syncthreads();
        const int jmax = (int)(N - j0 < SP_TJ ? N - j0 : SP_TJ);
        const double *pr = &sr[0][grp * SP_TB];
#pragma unroll 2
        for (int jj = 0; jj < jmax; ++jj) {
            const int w = kk + SP_TJ - 1 - jj;
            const double av = ta[w];
#pragma unroll
            for (int i = 0; i < SP_TB; ++i) rad[i] = fma(pr[jj * RB + i], av, rad[i]);
            if constexpr (HAS_C) {
                const double *pc = &sc[0][grp * SP_TB];
                const double gv = tg[w];
#pragma unroll
                for (int i = 0; i < SP_TB; ++i) cen[i] = fma(pc[jj * RB + i], gv, cen[i]);
            }
        }
        __syncthreads();
    }
    if (k >= N) return;

    double g4[4];
    if constexpr (MODE == MODE_RECIPE) {            // c_j != 0 only at j = 0, 1, 2, N - 1
        g4[0] = a.g[k];
        g4[1] = a.g[wrap(k - 1, N)];
        g4[2] = a.g[wrap(k - 2, N)];
        g4[3] = a.g[wrap(k + 1, N)];
    }
#pragma unroll
    for (int i = 0; i < SP_TB; ++i) {
        const int row = grp * SP_TB + i;
        const long long b = row0 + row;
        if (b >= B) break;
        double c = cen[i];
        if constexpr (MODE == MODE_RECIPE) {
            c = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) c = fma(cedge[row][e], g4[e], c);
        }
        const double r = rad[i];
        const bool ok = isfinite(c) && isfinite(r) && !bad[row];
        a.lo[b * N + k] = ok ? c - r : (double)NAN;
        a.hi[b * N + k] = ok ? c + r : (double)NAN;
    }
}

template <int MODE>
int launch(SpArgs &a, hipStream_t st)
{
    const int TK = a.N <= 64 ? 64 : a.N <= 128 ? 128 : 256;
    const long long RB = (long long)SP_TB * (SP_BLOCK / TK);
    a.tiles = (a.N + TK - 1) / TK;
    const long long nblocks = a.tiles * ((a.B + RB - 1) / RB);
    if (nblocks > 0x7fffffffLL) return PRE_E_SHAPE;
    const dim3 grid((unsigned)nblocks), block(SP_BLOCK);
    switch (TK) {
    case 64: hipLaunchKernelGGL((setprop_kernel<64, MODE>), grid, block, 0, st, a); break;
    case 128: hipLaunchKernelGGL((setprop_kernel<128, MODE>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((setprop_kernel<256, MODE>), grid, block, 0, st, a); break;
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int pre_setprop_abi_version(void) { return PRE_SETPROP_ABI_VERSION; }

int pre_setprop_bounds_f64(const void *centre, const int64_t c_strides[2], const void *radius, const int64_t r_strides[2],
                           int64_t B, int64_t N, const double *g, const double *a, double *lower, double *upper, int flags,
                           void *stream)
{
    if (B < 0 || N < 0 || !c_strides || !r_strides) return PRE_E_NULL;
    if (N < 1) return PRE_E_SHAPE;
    if (B == 0) return PRE_OK;
    if (!centre || !radius || !g || !a || !lower || !upper) return PRE_E_NULL;
    SpArgs s = {};
    s.c = centre;
    s.cB = c_strides[0];
    s.cT = c_strides[1];
    s.r = radius;
    s.rB = r_strides[0];
    s.rT = r_strides[1];
    s.g = g;
    s.a = a;
    s.lo = lower;
    s.hi = upper;
    s.B = B;
    s.N = N;
    hipStream_t st = (hipStream_t)stream;
    return (flags & PRE_SETPROP_FLAG_F64) ? launch<MODE_F64>(s, st) : launch<MODE_F32>(s, st);
}

int pre_setprop_recipe_f32(const float *field, const int64_t f_strides[2], int64_t B, int64_t Nt, const double *taps, int k,
                           const float *qhat, const int64_t q_strides[2], const double *g, const double *a, double *lower,
                           double *upper, int flags, void *stream)
{
    if (B < 0 || Nt < 0 || !f_strides || !taps) return PRE_E_NULL;
    if (Nt < 3) return PRE_E_SHAPE;
    if (k < 1 || k > PRE_SETPROP_MAX_TAPS || k > Nt + 2) return PRE_E_UNSUPPORTED;
    const int corr = (flags & PRE_SETPROP_FLAG_CORRELATION) ? 1 : 0;
    if (qhat) {
        if (!q_strides) return PRE_E_NULL;
        if (k % 2 == 0) return PRE_E_UNSUPPORTED;
        if (!corr)
            for (int i = 0; i < k / 2; ++i)
                if (taps[i] != taps[k - 1 - i]) return PRE_E_UNSUPPORTED;
    }
    if (B == 0) return PRE_OK;
    if (!field || !g || !a || !lower || !upper) return PRE_E_NULL;
    SpArgs s = {};
    s.f = field;
    s.fB = f_strides[0];
    s.fT = f_strides[1];
    s.q = qhat;
    s.qB = qhat ? q_strides[0] : 0;
    s.qT = qhat ? q_strides[1] : 0;
    for (int i = 0; i < k; ++i) s.taps[i] = taps[i];
    s.k = k;
    s.corr = corr;
    s.qshift = corr ? (k - 3) / 2 : -(k + 1) / 2;
    s.g = g;
    s.a = a;
    s.lo = lower;
    s.hi = upper;
    s.B = B;
    s.N = Nt + 1;
    return launch<MODE_RECIPE>(s, (hipStream_t)stream);
}

}  // extern "C"
