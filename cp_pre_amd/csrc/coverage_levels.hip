// Coverage at up to 16 calibration levels in one pass over the test residual (include/cp_pre_cov.h): the reference's
// `for alpha ...: calibrate; emp_cov` loop (Marginal/NS_Residuals_CP.py:308-312, 333-337) without one pass per level.
//
// Work split: a TILE is G = 64 samples x 256 cells; a thread owns one cell of it, computes that cell's half-widths hw_k once
// (nk registers) and streams the tile's samples past them, eight loads in flight.  A workgroup walks a contiguous run of
// cell chunks for one sample group, so per-workgroup state covers a long run of cells before it touches global memory:
//   marginal: the inside test of a wave is one v_cmp per level into an SGPR pair, counted by s_bcnt1 + s_add (no per-lane
//             counters: 1 VALU + 2 SALU per element and level without a centre, 3 + 3 with one); one 64-bit atomic per
//             level per workgroup at the end;
//   joint:    a wave whose ballot of "outside" is non-zero marks (level, sample) in LDS; the workgroup clears the marked
//             bytes of `inside` once, after its whole run of cells.
// Without a centre, y >= -hw && y <= hw is |y| <= hw exactly (NaN, negative hw and +-0 included): one compare per level,
// the |.| a source modifier.  With a centre the bounds are one packed add (c, c) + (-hw, hw) per level.
//
// This file is compiled with -ffp-contract=off (csrc/Makefile): hw = q * m and c - hw round as numpy's fp32 operations.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cp_pre_cov.h"
#include "../../include/cp_pre_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int COV_BLOCK = 256;     // cells per chunk: one per thread
constexpr int COV_G = 64;          // samples per group
constexpr int COV_UNROLL = 8;      // loads in flight per thread
constexpr long long COV_TARGET_BLOCKS = 2048;

typedef float f2 __attribute__((ext_vector_type(2)));

struct CovArgs {
    const float *y;
    long long ysN, ysA, ysB;
    const float *c;
    long long csN, csA, csB;
    long long n;
    int A, B, C, M;
    const float *q;
    long long q_ld;
    const float *m;
    unsigned long long *count;
    uint8_t *inside;
    long long inside_ld;
    int groups, chunks;
};

template <int NK, bool CENTRE, bool JOINT>
__global__ void __launch_bounds__(COV_BLOCK) cov_levels_kernel(const CovArgs a)
{
    __shared__ unsigned char flags[JOINT ? NK * COV_G : 1];
    __shared__ unsigned long long red[JOINT ? 1 : NK][COV_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    // this workgroup's run of cell chunks (the same for every sample group it visits)
    const int ch0 = (int)((long long)a.chunks * blockIdx.x / gridDim.x);
    const int ch1 = (int)((long long)a.chunks * (blockIdx.x + 1) / gridDim.x);
    unsigned long long tot[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) tot[k] = 0;

    for (int g = blockIdx.y; g < a.groups; g += gridDim.y) {
        const long long s0 = (long long)g * COV_G;
        const int ns = (int)min((long long)COV_G, a.n - s0);
        if (JOINT) {
            for (int i = tid; i < NK * COV_G; i += COV_BLOCK) flags[i] = 0;
            __syncthreads();
        }
        for (int ch = ch0; ch < ch1; ++ch) {
            const int j = ch * COV_BLOCK + tid;
            const bool valid = j < a.M;
            const int jj = valid ? j : 0;
            const int x = jj % a.C, t = jj / a.C, b = t % a.B, aa = t / a.B;
            const float *py = a.y + (aa * a.ysA + b * a.ysB + x) + s0 * a.ysN;
            const float *pc = CENTRE ? a.c + (aa * a.csA + b * a.csB + x) + s0 * a.csN : nullptr;
            const float mm = a.m ? a.m[jj] : 1.0f;
            float hw[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const float qk = a.q_ld ? a.q[k * a.q_ld + jj] : a.q[k];
                hw[k] = a.m ? qk * mm : qk;
            }
            f2 nh[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) nh[k] = (f2){-hw[k], hw[k]};
            unsigned cnt[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) cnt[k] = 0;

            // (lanes past the last cell sit the chunk out: a ballot counts active lanes only)
            if (valid) {
                auto test = [&](float v, float cv, int s) __attribute__((always_inline)) {
#pragma unroll
                    for (int k = 0; k < NK; ++k) {
                        // llvm.amdgcn.fcmp: the wave's compare mask straight into an SGPR pair (inactive lanes: 0).
                        // Predicates: 3 ordered >=, 5 ordered <=, 10 unordered >, 12 unordered <.
                        unsigned long long in;
                        if (CENTRE) {
                            const f2 lh = (f2){cv, cv} + nh[k];
                            in = JOINT ? (__builtin_amdgcn_fcmpf(v, lh.x, 12) | __builtin_amdgcn_fcmpf(v, lh.y, 10))
                                       : (__builtin_amdgcn_fcmpf(v, lh.x, 3) & __builtin_amdgcn_fcmpf(v, lh.y, 5));
                        } else {
                            in = __builtin_amdgcn_fcmpf(fabsf(v), hw[k], JOINT ? 10 : 5);
                        }
                        if (JOINT) {
                            if (in) flags[k * COV_G + s] = 1;           // (`in` holds the lanes OUTSIDE here)
                        } else {
                            cnt[k] += (unsigned)__popcll(in);
                        }
                    }
                };
                int s = 0;
                for (; s + COV_UNROLL <= ns; s += COV_UNROLL) {
                    float v[COV_UNROLL], cv[COV_UNROLL];
#pragma unroll
                    for (int u = 0; u < COV_UNROLL; ++u) {
                        v[u] = py[(long long)(s + u) * a.ysN];
                        cv[u] = CENTRE ? pc[(long long)(s + u) * a.csN] : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < COV_UNROLL; ++u) test(v[u], cv[u], s + u);
                }
                for (; s < ns; ++s) test(py[(long long)s * a.ysN], CENTRE ? pc[(long long)s * a.csN] : 0.0f, s);
            }
            if (!JOINT) {
#pragma unroll
                for (int k = 0; k < NK; ++k) tot[k] += lane == 0 ? cnt[k] : 0u;     // (per lane: kept out of the SGPRs)
            }
        }
        if (JOINT) {
            __syncthreads();
            for (int i = tid; i < NK * COV_G; i += COV_BLOCK) {
                const int k = i / COV_G, sl = i % COV_G;
                if (flags[i] && sl < ns) a.inside[k * a.inside_ld + s0 + sl] = 0;
            }
            __syncthreads();
        }
    }
    if (!JOINT) {
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NK; ++k) red[k][tid >> 6] = tot[k];
        }
        __syncthreads();
        if (tid < NK) {
            unsigned long long sum = 0;
#pragma unroll
            for (int w = 0; w < COV_BLOCK / 64; ++w) sum += red[tid][w];
            if (sum) atomicAdd(a.count + tid, sum);
        }
    }
}

template <int NK>
hipError_t launch_nk(const CovArgs &a, dim3 grid, hipStream_t st)
{
    const bool centre = a.c != nullptr, joint = a.inside != nullptr;
    if (centre && joint) hipLaunchKernelGGL((cov_levels_kernel<NK, true, true>), grid, dim3(COV_BLOCK), 0, st, a);
    else if (centre) hipLaunchKernelGGL((cov_levels_kernel<NK, true, false>), grid, dim3(COV_BLOCK), 0, st, a);
    else if (joint) hipLaunchKernelGGL((cov_levels_kernel<NK, false, true>), grid, dim3(COV_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((cov_levels_kernel<NK, false, false>), grid, dim3(COV_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch(const CovArgs &a, int nk, dim3 grid, hipStream_t st)
{
    switch (nk) {
#define COV_CASE(K) case K: return launch_nk<K>(a, grid, st);
        COV_CASE(1) COV_CASE(2) COV_CASE(3) COV_CASE(4) COV_CASE(5) COV_CASE(6) COV_CASE(7) COV_CASE(8)
        COV_CASE(9) COV_CASE(10) COV_CASE(11) COV_CASE(12) COV_CASE(13) COV_CASE(14) COV_CASE(15) COV_CASE(16)
#undef COV_CASE
    }
    return hipErrorInvalidValue;
}

}  // namespace

static_assert(PRE_COV_MAX_LEVELS == 16, "launch() instantiates 1..16 levels");

extern "C" {

int pre_cov_abi_version(void) { return PRE_COV_ABI_VERSION; }

int pre_cov_levels_f32(const float *y, int64_t y_sN, int64_t y_sA, int64_t y_sB,
                       const float *c, int64_t c_sN, int64_t c_sA, int64_t c_sB,
                       int64_t n, int64_t A, int64_t B, int64_t C,
                       const float *q, int64_t q_ld, const float *m, int nk,
                       uint64_t *count, uint8_t *inside, int64_t inside_ld, void *stream)
{
    if (!y || !q || nk <= 0 || n <= 0 || A <= 0 || B <= 0 || C <= 0 || q_ld < 0) return PRE_E_NULL;
    if ((count != nullptr) == (inside != nullptr) || (inside && inside_ld < n)) return PRE_E_NULL;
    const int64_t M = A * B * C;
    // flat cell indices and the per-cell offsets are int32 arithmetic in the kernel (a*sA etc. are promoted to 64 bits)
    if (M > 0x7fffffffLL - COV_BLOCK || (q_ld && q_ld < M)) return PRE_E_SHAPE;
    const long long groups = (n + COV_G - 1) / COV_G, chunks = (M + COV_BLOCK - 1) / COV_BLOCK;
    if (groups > 0x7fffffffLL) return PRE_E_SHAPE;
    long long splits = (COV_TARGET_BLOCKS + groups - 1) / groups;
    splits = splits < 1 ? 1 : (splits > chunks ? chunks : splits);
    const long long gy = groups < 65535 ? groups : 65535;
    CovArgs a{y, y_sN, y_sA, y_sB, c, c_sN, c_sA, c_sB, n, (int)A, (int)B, (int)C, (int)M, q, q_ld, m,
              reinterpret_cast<unsigned long long *>(count), inside, inside_ld, (int)groups, (int)chunks};
    for (int k0 = 0; k0 < nk; k0 += PRE_COV_MAX_LEVELS) {
        const int kn = (nk - k0) < PRE_COV_MAX_LEVELS ? (nk - k0) : PRE_COV_MAX_LEVELS;
        CovArgs ak = a;
        ak.q = q + (q_ld ? k0 * q_ld : k0);
        if (count) ak.count = a.count + k0;
        if (inside) ak.inside = inside + k0 * inside_ld;
        const hipError_t e = launch(ak, kn, dim3((unsigned)splits, (unsigned)gy), (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    return PRE_OK;
}

}  // extern "C"
