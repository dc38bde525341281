// Bounds on the solution by sample acceptance (include/cp_pre_bounds.h): the per-cell envelope (min, max) of the candidate
// fields u_s whose residual lies inside the calibrated set, at up to 16 levels per launch and one read of u (and r).
//
// Work split (envelope and cellwise passes): a workgroup of 256 threads is R rows x W cells, W = 256 / 128 / 64 as the
// sample has > 128 / > 64 / fewer cells, so every wave covers W consecutive cells of ONE sample at a time: the sample index,
// and with it the sample's acceptance bits, are wave-uniform.  A thread owns one cell and streams its row's samples past
// its per-level registers, eight loads in flight.  Wide inputs (many cells) give every workgroup its own cells and all
// samples: the thread merges its registers into lo / hi itself.  Tall inputs (few cells, many samples) also split the
// samples over S workgroups; each (split, row) then writes partial bounds to the workspace, and fold_kernel merges them 64
// at a time (two launches for up to 4096 partials), exactly, into lo / hi / count.  Partials + fold rather than ordered-int
// atomics: a tall shape puts thousands of workgroups on each of a few hundred cells, and same-address atomics from all of
// them would serialise; the fold is a dense read of 8 B per partial (a few % of u's bytes at the ODE shape).
//
// Envelope: a prepass packs the accept flags of each sample into a bit mask (and counts the accepted samples per level).
// The main pass tests the mask in scalar registers: a run of levels that ends at the last level (nested levels whose sets
// grow with k) updates one register pair, that of the run's first level; a run that starts at level 0 (sets that shrink
// with k) that of its last level; the epilogue folds the first kind forwards and the second backwards over the levels.
// Other masks update one pair per accepting level.  min / max are v_minimum3 / v_maximum3 (NaN-propagating, as np.min).
//
// Cellwise: per element and level one compare (|r| <= hw without a centre, two with bounds) and a masked min / max / count.
// Rowcount: coverage_levels.hip's tile (64 samples x 256 cells per workgroup iteration), the per-wave inside count of each
// (level, sample) added into LDS and flushed with one atomic per (level, sample) per workgroup.
//
// This file is compiled with -ffp-contract=off (csrc/Makefile): hw = q * m and c -+ hw round as numpy's fp32 operations.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cp_pre_bounds.h"
#include "../../include/cp_pre_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLK = 256;               // threads per workgroup
constexpr int UNR = 8;                 // loads in flight per thread
constexpr long long TARGET_BLOCKS = 1024;
constexpr long long MIN_PER_ROW = 64;  // samples per row of a split, at least
constexpr int FOLD = 64;               // partials merged per fold workgroup
constexpr int RC_G = 64;               // rowcount: samples per group
constexpr long long RC_TARGET_BLOCKS = 2048;

__device__ __forceinline__ float vmin(float a, float b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ float vmax(float a, float b) { return __builtin_elementwise_maximum(a, b); }

// The launch geometry of one shape: every entry point and its workspace query derive it from (n, M) alone.
struct Plan {
    int cw_log, rows;        // W = 1 << cw_log cells per row, rows = 256 / W
    long long chunks;        // cell chunks of W
    long long S, per;        // sample splits and samples per split
    long long P;             // partial slots: S * rows (1: no workspace)
};

Plan make_plan(long long n, long long M)
{
    Plan p;
    p.cw_log = M > 128 ? 8 : (M > 64 ? 7 : 6);
    p.rows = BLK >> p.cw_log;
    p.chunks = (M + (1 << p.cw_log) - 1) >> p.cw_log;
    long long S = (TARGET_BLOCKS + p.chunks - 1) / p.chunks;
    const long long smax = (n + p.rows * MIN_PER_ROW - 1) / (p.rows * MIN_PER_ROW);
    S = S < smax ? S : smax;
    S = S < 1 ? 1 : (S > 4096 / p.rows ? 4096 / p.rows : S);
    p.per = (n + S - 1) / S;
    p.S = (n + p.per - 1) / p.per;            // no empty split
    p.P = p.S * p.rows;
    return p;
}

long long align_up(long long x) { return (x + 255) & ~255LL; }

// workspace: [mask bits: n uint32] (envelope) + partial lo, hi [P][nk][M] fp32 (+ count int32, cellwise) + the second fold
// level [ceil(P / 64)][nk][M] of the same; nothing when P == 1
long long workspace_bytes(const Plan &p, long long n, long long M, int nkl, bool envelope, bool cellwise)
{
    long long b = envelope ? align_up(n * 4) : 0;
    if (p.P > 1) {
        const long long per = (long long)nkl * M * (cellwise ? 12 : 8);
        const long long p2 = (p.P + FOLD - 1) / FOLD;
        b += align_up(p.P * per) + (p2 > 1 ? align_up(p2 * per) : 0);
    }
    return b;
}

// ------------------------------------------------------------------ envelope
__global__ void __launch_bounds__(BLK) mask_kernel(const uint8_t *acc, long long ld, int nk, long long n, unsigned *bits,
                                                   unsigned long long *count)
{
    __shared__ unsigned red[PRE_BOUNDS_MAX_LEVELS];
    const int tid = threadIdx.x;
    if (tid < PRE_BOUNDS_MAX_LEVELS) red[tid] = 0;
    __syncthreads();
    unsigned cnt[PRE_BOUNDS_MAX_LEVELS];
#pragma unroll
    for (int k = 0; k < PRE_BOUNDS_MAX_LEVELS; ++k) cnt[k] = 0;
    for (long long s = (long long)blockIdx.x * BLK + tid; s < n; s += (long long)gridDim.x * BLK) {
        unsigned m = 0;
#pragma unroll
        for (int k = 0; k < PRE_BOUNDS_MAX_LEVELS; ++k)
            if (k < nk && acc[k * ld + s]) m |= 1u << k;
        bits[s] = m;
#pragma unroll
        for (int k = 0; k < PRE_BOUNDS_MAX_LEVELS; ++k) cnt[k] += (m >> k) & 1u;
    }
#pragma unroll
    for (int k = 0; k < PRE_BOUNDS_MAX_LEVELS; ++k)
        if (k < nk && cnt[k]) atomicAdd(&red[k], cnt[k]);
    __syncthreads();
    if (tid < nk && red[tid]) atomicAdd(count + tid, (unsigned long long)red[tid]);
}

struct EnvArgs {
    const float *u;
    long long sN, sA, sB;
    long long n, per;
    int A, B, C, M, cw_log;
    const unsigned *bits;
    float *lo, *hi;            // [NK][M] of this launch
    float *plo, *phi;          // partials [P][NK][M]; NULL: merge into lo / hi
};

template <int NK>
__global__ void __launch_bounds__(BLK) envelope_kernel(const EnvArgs a)
{
    const int tid = threadIdx.x;
    const int rows = BLK >> a.cw_log;
    const int row = __builtin_amdgcn_readfirstlane(tid >> a.cw_log);      // wave-uniform (W >= 64)
    const int j = (int)blockIdx.x * (1 << a.cw_log) + (tid & ((1 << a.cw_log) - 1));
    const bool valid = j < a.M;
    const int jj = valid ? j : 0;             // lanes past the last cell read cell 0 and store nothing
    const int x = jj % a.C, t = jj / a.C, b = t % a.B, aa = t / a.B;
    const float *pu = a.u + (aa * a.sA + b * a.sB + x);
    const long long s0 = (long long)blockIdx.y * a.per;
    const long long s1 = min(a.n, s0 + a.per);

    float Rl[NK], Rh[NK], Al[NK], Ah[NK], Dl[NK], Dh[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        Rl[k] = Al[k] = Dl[k] = __builtin_inff();
        Rh[k] = Ah[k] = Dh[k] = -__builtin_inff();
    }
    constexpr unsigned FULL = (1u << NK) - 1u;
    // (one scalar switch on the run's level instead of a chain of NK compares and branches)
#define ENV_PAIR(P, K)                                                                                           \
    case K:                                                                                                      \
        if constexpr (K < NK) { P##l[K] = vmin(P##l[K], v); P##h[K] = vmax(P##h[K], v); }                      \
        break;
#define ENV_SWITCH(P, f)                                                                                         \
    switch (f) {                                                                                                 \
        ENV_PAIR(P, 0) ENV_PAIR(P, 1) ENV_PAIR(P, 2) ENV_PAIR(P, 3) ENV_PAIR(P, 4) ENV_PAIR(P, 5)                 \
        ENV_PAIR(P, 6) ENV_PAIR(P, 7) ENV_PAIR(P, 8) ENV_PAIR(P, 9) ENV_PAIR(P, 10) ENV_PAIR(P, 11)              \
        ENV_PAIR(P, 12) ENV_PAIR(P, 13) ENV_PAIR(P, 14) ENV_PAIR(P, 15)                                          \
    }
    auto upd = [&](float v, unsigned m) __attribute__((always_inline)) {
        if (m == 0u) return;
        const unsigned low = m & (0u - m);
        if (m + low == FULL + 1u) {                      // levels f .. NK-1: register pair of f
            ENV_SWITCH(A, __builtin_ctz(m))
        } else if ((m & (m + 1u)) == 0u) {               // levels 0 .. t: register pair of t
            ENV_SWITCH(D, 31 - __builtin_clz(m))
        } else {                                         // any other set of levels
#pragma unroll
            for (int k = 0; k < NK; ++k)
                if (m & (1u << k)) { Rl[k] = vmin(Rl[k], v); Rh[k] = vmax(Rh[k], v); }
        }
    };
    long long s = s0 + row;
    for (; s + (long long)(UNR - 1) * rows < s1; s += (long long)UNR * rows) {
        unsigned m[UNR];
        float v[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) m[u] = a.bits[s + u * rows];
        // (unconditional: a load behind a branch on its sample's mask would wait for the mask's scalar load first)
#pragma unroll
        for (int u = 0; u < UNR; ++u) v[u] = __builtin_nontemporal_load(pu + (s + u * rows) * a.sN);
#pragma unroll
        for (int u = 0; u < UNR; ++u) upd(v[u], m[u]);
    }
    for (; s < s1; s += rows) {
        const unsigned m = a.bits[s];
        if (m) upd(pu[s * a.sN], m);
    }
    // level k: its own updates, the "from f" runs with f <= k, the "up to t" runs with t >= k
    float rl = __builtin_inff(), rh = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        rl = vmin(rl, Al[k]); rh = vmax(rh, Ah[k]);
        Rl[k] = vmin(Rl[k], rl); Rh[k] = vmax(Rh[k], rh);
    }
    rl = __builtin_inff(); rh = -__builtin_inff();
#pragma unroll
    for (int k = NK - 1; k >= 0; --k) {
        rl = vmin(rl, Dl[k]); rh = vmax(rh, Dh[k]);
        Rl[k] = vmin(Rl[k], rl); Rh[k] = vmax(Rh[k], rh);
    }
    if (!valid) return;
    if (a.plo) {
        const long long base = ((long long)blockIdx.y * rows + row) * NK * a.M + j;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            a.plo[base + (long long)k * a.M] = Rl[k];
            a.phi[base + (long long)k * a.M] = Rh[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const long long i = (long long)k * a.M + j;
            a.lo[i] = vmin(a.lo[i], Rl[k]);
            a.hi[i] = vmax(a.hi[i], Rh[k]);
        }
    }
}

// ------------------------------------------------------------------ cellwise
struct CellArgs {
    const float *u;
    long long usN, usA, usB;
    const float *r;
    long long rsN, rsA, rsB;
    long long n, per;
    int A, B, C, M, cw_log;
    const float *q;
    long long q_ld;
    const float *m, *c, *blo, *bhi;      // (all per level / cell in flat order, already offset to this launch's levels)
    float *lo, *hi;
    int *cnt;
    float *plo, *phi;
    int *pcnt;
};

template <int NK, bool ABS>
__global__ void __launch_bounds__(BLK) cellwise_kernel(const CellArgs a)
{
    const int tid = threadIdx.x;
    const int rows = BLK >> a.cw_log;
    const int row = __builtin_amdgcn_readfirstlane(tid >> a.cw_log);
    const int j = (int)blockIdx.x * (1 << a.cw_log) + (tid & ((1 << a.cw_log) - 1));
    const bool valid = j < a.M;
    const int jj = valid ? j : 0;
    const int x = jj % a.C, t = jj / a.C, b = t % a.B, aa = t / a.B;
    const float *pu = a.u + (aa * a.usA + b * a.usB + x);
    const float *pr = a.r + (aa * a.rsA + b * a.rsB + x);
    const long long s0 = (long long)blockIdx.y * a.per;
    const long long s1 = min(a.n, s0 + a.per);

    // ABS: |r| <= hw (no centre, no given bounds; exact, NaN and a negative hw included); else bl <= r <= bh
    float bl[NK], bh[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (a.blo) {
            bl[k] = a.blo[(long long)k * a.M + jj];
            bh[k] = a.bhi[(long long)k * a.M + jj];
        } else {
            const float qk = a.q_ld ? a.q[k * a.q_ld + jj] : a.q[k];
            const float hw = a.m ? qk * a.m[jj] : qk;
            const float cc = a.c ? a.c[jj] : 0.0f;
            bl[k] = a.c ? cc - hw : -hw;
            bh[k] = a.c ? cc + hw : hw;
        }
    }
    float L[NK], H[NK];
    int N[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) { L[k] = __builtin_inff(); H[k] = -__builtin_inff(); N[k] = 0; }
    auto upd = [&](float v, float w) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const bool in = ABS ? (fabsf(w) <= bh[k]) : (w >= bl[k] && w <= bh[k]);
            L[k] = in ? vmin(L[k], v) : L[k];
            H[k] = in ? vmax(H[k], v) : H[k];
            N[k] += in ? 1 : 0;
        }
    };
    long long s = s0 + row;
    for (; s + (long long)(UNR - 1) * rows < s1; s += (long long)UNR * rows) {
        float v[UNR], w[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            v[u] = __builtin_nontemporal_load(pu + (s + u * rows) * a.usN);
            w[u] = __builtin_nontemporal_load(pr + (s + u * rows) * a.rsN);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) upd(v[u], w[u]);
    }
    for (; s < s1; s += rows) upd(pu[s * a.usN], pr[s * a.rsN]);
    if (!valid) return;
    if (a.plo) {
        const long long base = ((long long)blockIdx.y * rows + row) * NK * a.M + j;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            a.plo[base + (long long)k * a.M] = L[k];
            a.phi[base + (long long)k * a.M] = H[k];
            a.pcnt[base + (long long)k * a.M] = N[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const long long i = (long long)k * a.M + j;
            a.lo[i] = vmin(a.lo[i], L[k]);
            a.hi[i] = vmax(a.hi[i], H[k]);
            a.cnt[i] += N[k];
        }
    }
}

// ------------------------------------------------------------------ fold of partials: [P][KM] -> [ceil(P/64)][KM] or the outputs
// A workgroup is 64 columns x 4 partial lanes; workgroup (x, y) folds partials [64y, 64y + 64) of its 64 columns.
__global__ void __launch_bounds__(BLK) fold_kernel(const float *plo, const float *phi, const int *pcnt, long long P, long long KM,
                                                   float *dlo, float *dhi, int *dcnt, int merge)
{
    __shared__ float sl[4][64], sh[4][64];
    __shared__ int sc[4][64];
    const int tid = threadIdx.x, col = tid & 63, pl = tid >> 6;
    const long long i = (long long)blockIdx.x * 64 + col;
    const long long p0 = (long long)blockIdx.y * FOLD, p1 = min(P, p0 + FOLD);
    float l = __builtin_inff(), h = -__builtin_inff();
    int c = 0;
    if (i < KM) {
        for (long long p = p0 + pl; p < p1; p += 4) {
            l = vmin(l, plo[p * KM + i]);
            h = vmax(h, phi[p * KM + i]);
            if (pcnt) c += pcnt[p * KM + i];
        }
    }
    sl[pl][col] = l; sh[pl][col] = h; sc[pl][col] = c;
    __syncthreads();
    if (pl != 0 || i >= KM) return;
#pragma unroll
    for (int w = 1; w < 4; ++w) { l = vmin(l, sl[w][col]); h = vmax(h, sh[w][col]); c += sc[w][col]; }
    if (merge) {
        dlo[i] = vmin(dlo[i], l);
        dhi[i] = vmax(dhi[i], h);
        if (dcnt) dcnt[i] += c;
    } else {
        const long long o = (long long)blockIdx.y * KM + i;
        dlo[o] = l; dhi[o] = h;
        if (dcnt) dcnt[o] = c;
    }
}

// partials [P][KM] at plo / phi / pcnt (scratch for the second level after them) -> merged into lo / hi / cnt
hipError_t fold(float *plo, float *phi, int *pcnt, long long P, long long KM, float *lo, float *hi, int *cnt, hipStream_t st)
{
    const long long P2 = (P + FOLD - 1) / FOLD;
    const unsigned gx = (unsigned)((KM + 63) / 64);
    if (P2 == 1) {
        hipLaunchKernelGGL(fold_kernel, dim3(gx, 1), dim3(BLK), 0, st, plo, phi, pcnt, P, KM, lo, hi, cnt, 1);
        return hipGetLastError();
    }
    // second level right after the first: [P2][KM] lo, hi (, count)
    float *qlo = pcnt ? reinterpret_cast<float *>(pcnt + P * KM) : phi + P * KM;
    float *qhi = qlo + P2 * KM;
    int *qcnt = pcnt ? reinterpret_cast<int *>(qhi + P2 * KM) : nullptr;
    hipLaunchKernelGGL(fold_kernel, dim3(gx, (unsigned)P2), dim3(BLK), 0, st, plo, phi, pcnt, P, KM, qlo, qhi, qcnt, 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fold_kernel, dim3(gx, 1), dim3(BLK), 0, st, qlo, qhi, qcnt, P2, KM, lo, hi, cnt, 1);
    return hipGetLastError();
}

// ------------------------------------------------------------------ rowcount (coverage_levels.hip's tile, per-sample counts)
struct RcArgs {
    const float *y;
    long long ysN, ysA, ysB;
    const float *c;
    long long csN, csA, csB;
    long long n;
    int A, B, C, M;
    const float *q;
    long long q_ld;
    const float *m;
    unsigned *counts;
    long long counts_ld;
    int groups, chunks;
};

typedef float f2 __attribute__((ext_vector_type(2)));

template <int NK, bool CENTRE>
__global__ void __launch_bounds__(BLK) rowcount_kernel(const RcArgs a)
{
    __shared__ unsigned cnt[NK * RC_G];
    const int tid = threadIdx.x, lane = tid & 63;
    const int ch0 = (int)((long long)a.chunks * blockIdx.x / gridDim.x);
    const int ch1 = (int)((long long)a.chunks * (blockIdx.x + 1) / gridDim.x);
    for (int g = blockIdx.y; g < a.groups; g += gridDim.y) {
        const long long s0 = (long long)g * RC_G;
        const int ns = (int)min((long long)RC_G, a.n - s0);
        for (int i = tid; i < NK * RC_G; i += BLK) cnt[i] = 0;
        __syncthreads();
        for (int ch = ch0; ch < ch1; ++ch) {
            const int j = ch * BLK + tid;
            const bool valid = j < a.M;
            const int jj = valid ? j : 0;
            const int x = jj % a.C, t = jj / a.C, b = t % a.B, aa = t / a.B;
            const float *py = a.y + (aa * a.ysA + b * a.ysB + x) + s0 * a.ysN;
            const float *pc = CENTRE ? a.c + (aa * a.csA + b * a.csB + x) + s0 * a.csN : nullptr;
            const float mm = a.m ? a.m[jj] : 1.0f;
            float hw[NK];
            f2 nh[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const float qk = a.q_ld ? a.q[k * a.q_ld + jj] : a.q[k];
                hw[k] = a.m ? qk * mm : qk;
                nh[k] = (f2){-hw[k], hw[k]};
            }
            // (lanes past the last cell sit the chunk out: a ballot counts active lanes only; lane 0 is active whenever
            // any lane of its wave is)
            if (valid) {
                auto test = [&](float v, float cv, int s) __attribute__((always_inline)) {
#pragma unroll
                    for (int k = 0; k < NK; ++k) {
                        // predicates: 3 ordered >=, 5 ordered <=
                        unsigned long long in;
                        if (CENTRE) {
                            const f2 lh = (f2){cv, cv} + nh[k];
                            in = __builtin_amdgcn_fcmpf(v, lh.x, 3) & __builtin_amdgcn_fcmpf(v, lh.y, 5);
                        } else {
                            in = __builtin_amdgcn_fcmpf(fabsf(v), hw[k], 5);
                        }
                        const unsigned pc = (unsigned)__popcll(in);
                        if (lane == 0 && pc) atomicAdd(&cnt[k * RC_G + s], pc);
                    }
                };
                int s = 0;
                for (; s + UNR <= ns; s += UNR) {
                    float v[UNR], cv[UNR];
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        v[u] = py[(long long)(s + u) * a.ysN];
                        cv[u] = CENTRE ? pc[(long long)(s + u) * a.csN] : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < UNR; ++u) test(v[u], cv[u], s + u);
                }
                for (; s < ns; ++s) test(py[(long long)s * a.ysN], CENTRE ? pc[(long long)s * a.csN] : 0.0f, s);
            }
        }
        __syncthreads();
        for (int i = tid; i < NK * RC_G; i += BLK) {
            const int k = i / RC_G, sl = i % RC_G;
            if (cnt[i] && sl < ns) atomicAdd(a.counts + k * a.counts_ld + s0 + sl, cnt[i]);
        }
        __syncthreads();
    }
}

#define NK_SWITCH(nk, CALL)                                                                                      \
    switch (nk) {                                                                                                \
        case 1: CALL(1) case 2: CALL(2) case 3: CALL(3) case 4: CALL(4)                                          \
        case 5: CALL(5) case 6: CALL(6) case 7: CALL(7) case 8: CALL(8)                                          \
        case 9: CALL(9) case 10: CALL(10) case 11: CALL(11) case 12: CALL(12)                                    \
        case 13: CALL(13) case 14: CALL(14) case 15: CALL(15) case 16: CALL(16)                                  \
    }

hipError_t launch_envelope(const EnvArgs &a, int nk, dim3 grid, hipStream_t st)
{
#define ENV_CALL(K) { hipLaunchKernelGGL((envelope_kernel<K>), grid, dim3(BLK), 0, st, a); return hipGetLastError(); }
    NK_SWITCH(nk, ENV_CALL)
#undef ENV_CALL
    return hipErrorInvalidValue;
}

hipError_t launch_cellwise(const CellArgs &a, int nk, bool abs_form, dim3 grid, hipStream_t st)
{
#define CELL_CALL(K)                                                                                             \
    {                                                                                                            \
        if (abs_form) hipLaunchKernelGGL((cellwise_kernel<K, true>), grid, dim3(BLK), 0, st, a);                 \
        else hipLaunchKernelGGL((cellwise_kernel<K, false>), grid, dim3(BLK), 0, st, a);                         \
        return hipGetLastError();                                                                                \
    }
    NK_SWITCH(nk, CELL_CALL)
#undef CELL_CALL
    return hipErrorInvalidValue;
}

hipError_t launch_rowcount(const RcArgs &a, int nk, bool centre, dim3 grid, hipStream_t st)
{
#define RC_CALL(K)                                                                                               \
    {                                                                                                            \
        if (centre) hipLaunchKernelGGL((rowcount_kernel<K, true>), grid, dim3(BLK), 0, st, a);                   \
        else hipLaunchKernelGGL((rowcount_kernel<K, false>), grid, dim3(BLK), 0, st, a);                         \
        return hipGetLastError();                                                                                \
    }
    NK_SWITCH(nk, RC_CALL)
#undef RC_CALL
    return hipErrorInvalidValue;
}

// shape checks shared by the entry points: flat cell indices and per-cell offsets are int32 arithmetic in the kernels
int check_shape(int64_t n, int64_t A, int64_t B, int64_t C, int nk)
{
    if (nk <= 0 || n <= 0 || A <= 0 || B <= 0 || C <= 0) return PRE_E_NULL;
    if (A * B * C > 0x7fffffffLL - BLK) return PRE_E_SHAPE;
    return PRE_OK;
}

int min_levels(int nk) { return nk < PRE_BOUNDS_MAX_LEVELS ? nk : PRE_BOUNDS_MAX_LEVELS; }

}  // namespace

static_assert(PRE_BOUNDS_MAX_LEVELS == 16, "NK_SWITCH instantiates 1..16 levels");

extern "C" {

int pre_bounds_abi_version(void) { return PRE_BOUNDS_ABI_VERSION; }

int pre_bounds_envelope_workspace(int64_t n, int64_t A, int64_t B, int64_t C, int nk, int64_t *bytes)
{
    const int rc = check_shape(n, A, B, C, nk);
    if (rc != PRE_OK) return rc;
    if (!bytes) return PRE_E_NULL;
    const long long M = A * B * C;
    *bytes = workspace_bytes(make_plan(n, M), n, M, min_levels(nk), true, false);
    return PRE_OK;
}

int pre_bounds_cellwise_workspace(int64_t n, int64_t A, int64_t B, int64_t C, int nk, int64_t *bytes)
{
    const int rc = check_shape(n, A, B, C, nk);
    if (rc != PRE_OK) return rc;
    if (!bytes) return PRE_E_NULL;
    const long long M = A * B * C;
    *bytes = workspace_bytes(make_plan(n, M), n, M, min_levels(nk), false, true);
    return PRE_OK;
}

int pre_bounds_envelope_f32(const float *u, int64_t u_sN, int64_t u_sA, int64_t u_sB,
                            int64_t n, int64_t A, int64_t B, int64_t C,
                            const uint8_t *accept, int64_t accept_ld, int nk,
                            float *lo, float *hi, int64_t *count, void *work, int64_t work_bytes, void *stream)
{
    const int rc = check_shape(n, A, B, C, nk);
    if (rc != PRE_OK) return rc;
    if (!u || !accept || !lo || !hi || !count || accept_ld < n) return PRE_E_NULL;
    const long long M = A * B * C;
    const Plan p = make_plan(n, M);
    const int nkl = min_levels(nk);
    if (!work || work_bytes < workspace_bytes(p, n, M, nkl, true, false)) return PRE_E_NULL;
    hipStream_t st = (hipStream_t)stream;
    unsigned *bits = reinterpret_cast<unsigned *>(work);
    float *plo = reinterpret_cast<float *>(static_cast<char *>(work) + align_up(n * 4));
    for (int k0 = 0; k0 < nk; k0 += PRE_BOUNDS_MAX_LEVELS) {
        const int kn = min_levels(nk - k0);
        const long long mb = (n + BLK - 1) / BLK;
        hipLaunchKernelGGL(mask_kernel, dim3((unsigned)(mb < 256 ? mb : 256)), dim3(BLK), 0, st, accept + k0 * accept_ld,
                           (long long)accept_ld, kn, (long long)n, bits, reinterpret_cast<unsigned long long *>(count + k0));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        const long long KM = (long long)kn * M;
        EnvArgs a{u, u_sN, u_sA, u_sB, n, p.per, (int)A, (int)B, (int)C, (int)M, p.cw_log, bits,
                  lo + k0 * M, hi + k0 * M, p.P > 1 ? plo : nullptr, p.P > 1 ? plo + p.P * KM : nullptr};
        e = launch_envelope(a, kn, dim3((unsigned)p.chunks, (unsigned)p.S), st);
        if (e == hipSuccess && p.P > 1) e = fold(a.plo, a.phi, nullptr, p.P, KM, a.lo, a.hi, nullptr, st);
        if (e != hipSuccess) return (int)e;
    }
    return PRE_OK;
}

int pre_bounds_cellwise_f32(const float *u, int64_t u_sN, int64_t u_sA, int64_t u_sB,
                            const float *r, int64_t r_sN, int64_t r_sA, int64_t r_sB,
                            int64_t n, int64_t A, int64_t B, int64_t C,
                            const float *q, int64_t q_ld, const float *m, const float *c,
                            const float *blo, const float *bhi, int nk,
                            float *lo, float *hi, int32_t *count, void *work, int64_t work_bytes, void *stream)
{
    const int rc = check_shape(n, A, B, C, nk);
    if (rc != PRE_OK) return rc;
    if (!u || !r || !lo || !hi || !count || q_ld < 0) return PRE_E_NULL;
    const bool given = blo != nullptr;
    if (given ? (!bhi || q || m || c) : (!q || bhi)) return PRE_E_NULL;
    const long long M = A * B * C;
    if (q_ld && q_ld < M) return PRE_E_SHAPE;
    const Plan p = make_plan(n, M);
    const int nkl = min_levels(nk);
    const long long need = workspace_bytes(p, n, M, nkl, false, true);
    if (need && (!work || work_bytes < need)) return PRE_E_NULL;
    hipStream_t st = (hipStream_t)stream;
    for (int k0 = 0; k0 < nk; k0 += PRE_BOUNDS_MAX_LEVELS) {
        const int kn = min_levels(nk - k0);
        const long long KM = (long long)kn * M;
        float *plo = p.P > 1 ? static_cast<float *>(work) : nullptr;
        CellArgs a{u, u_sN, u_sA, u_sB, r, r_sN, r_sA, r_sB, n, p.per, (int)A, (int)B, (int)C, (int)M, p.cw_log,
                   given ? nullptr : q + (q_ld ? k0 * q_ld : k0), q_ld, m, c,
                   given ? blo + k0 * M : nullptr, given ? bhi + k0 * M : nullptr,
                   lo + k0 * M, hi + k0 * M, count + k0 * M,
                   plo, plo ? plo + p.P * KM : nullptr, plo ? reinterpret_cast<int *>(plo + 2 * p.P * KM) : nullptr};
        hipError_t e = launch_cellwise(a, kn, !given && !c, dim3((unsigned)p.chunks, (unsigned)p.S), st);
        if (e == hipSuccess && p.P > 1) e = fold(a.plo, a.phi, a.pcnt, p.P, KM, a.lo, a.hi, a.cnt, st);
        if (e != hipSuccess) return (int)e;
    }
    return PRE_OK;
}

int pre_bounds_rowcount_f32(const float *r, int64_t r_sN, int64_t r_sA, int64_t r_sB,
                            const float *c, int64_t c_sN, int64_t c_sA, int64_t c_sB,
                            int64_t n, int64_t A, int64_t B, int64_t C,
                            const float *q, int64_t q_ld, const float *m, int nk,
                            int32_t *counts, int64_t counts_ld, void *stream)
{
    const int rc = check_shape(n, A, B, C, nk);
    if (rc != PRE_OK) return rc;
    if (!r || !q || !counts || q_ld < 0 || counts_ld < n) return PRE_E_NULL;
    const long long M = A * B * C;
    if (q_ld && q_ld < M) return PRE_E_SHAPE;
    const long long groups = (n + RC_G - 1) / RC_G, chunks = (M + BLK - 1) / BLK;
    if (groups > 0x7fffffffLL) return PRE_E_SHAPE;
    long long splits = (RC_TARGET_BLOCKS + groups - 1) / groups;
    splits = splits < 1 ? 1 : (splits > chunks ? chunks : splits);
    const long long gy = groups < 65535 ? groups : 65535;
    RcArgs a{r, r_sN, r_sA, r_sB, c, c_sN, c_sA, c_sB, n, (int)A, (int)B, (int)C, (int)M, q, q_ld, m,
             reinterpret_cast<unsigned *>(counts), counts_ld, (int)groups, (int)chunks};
    for (int k0 = 0; k0 < nk; k0 += PRE_BOUNDS_MAX_LEVELS) {
        const int kn = min_levels(nk - k0);
        RcArgs ak = a;
        ak.q = q + (q_ld ? k0 * q_ld : k0);
        ak.counts = a.counts + k0 * counts_ld;
        const hipError_t e = launch_rowcount(ak, kn, c != nullptr, dim3((unsigned)splits, (unsigned)gy), (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    return PRE_OK;
}

}  // extern "C"
