// dist_select.hip - the device sweeps of the sharded marginal calibration by histogram exchange (include/cp_pre_dist.h;
// the protocol around them: cp_pre_amd/pipeline.py, _marginal_histogram).
//
// Bound: HBM.  Three sweeps read each local score once (window, histogram, collect); the pick reads only the candidates
// an owner received.  The sweeps share the column-tile shape of kth_axis0.hip: a 1024-thread workgroup owns 64 adjacent
// cells (256 B of every sample row), lane = cell, wave w takes rows w, w + 16, ... with DS_U loads in flight per lane.
// Counters live in LDS: 256 buckets x 64 cells of 16 bits = 32 KiB, cells c and c+32 sharing a word so that the 64 LDS
// atomics of a wave-instruction never hit the same counter (kth_axis0.hip:55-57); a workgroup flushes them to its own
// cells' words of the global histogram after at most 65535 rows - no global atomics anywhere, every result reproducible.
#include "common.h"
#include "../../include/cp_pre_dist.h"

namespace {

constexpr int DS_W = 64, DS_WAVES = 16, DS_T = DS_W * DS_WAVES, DS_U = 8;
constexpr int DS_NB = PRE_DIST_NB, DS_CHUNK = 65535;
constexpr int DS_PICK_CAP = PRE_DIST_PICK_CAP;

struct DistSrc { const float *s; long long PS, RS, n, per, c0, C, Co, Cp; };   // Cp = W * Co: the padded run

// first element of cell c of the run (c < C)
__device__ __forceinline__ const float *ds_col(const DistSrc &a, long long c)
{
    const long long g = a.c0 + c;
    const long long p = g / a.per;
    return a.s + p * a.PS + (g - p * a.per);
}

// f(v) for the rows r0 + wave, r0 + wave + 16, ... < r1 of one column
template <typename F>
__device__ __forceinline__ void ds_rows(const float *col, long long RS, long long r0, long long r1, int wave, F &&f)
{
    long long row = r0 + wave;
    const long long step = (long long)DS_WAVES * RS;
    const float *p = col + row * RS;
    for (; row + (long long)(DS_U - 1) * DS_WAVES < r1; row += (long long)DS_U * DS_WAVES) {
        float v[DS_U];
#pragma unroll
        for (int u = 0; u < DS_U; ++u) v[u] = p[u * step];
#pragma unroll
        for (int u = 0; u < DS_U; ++u) f(v[u]);
        p += DS_U * step;
    }
    for (; row < r1; row += DS_WAVES) {
        f(*p);
        p += step;
    }
}

struct DsMap {
    uint32_t klo;
    float vlo, sf;
    int sh;       // < 0: the cell takes no part
    __device__ __forceinline__ void load(const int32_t *params, long long Cp, long long c)
    {
        klo = (uint32_t)params[c];
        sf = __int_as_float(params[Cp + c]);
        sh = params[2 * Cp + c];
        vlo = key2f(klo);
    }
    // monotone in the key order: value-linear (fp32, the file is built without contraction) or key-linear
    __device__ __forceinline__ int bucket(float v) const
    {
        if (sf > 0.0f) {
            const float t = (v - vlo) * sf;
            return t >= (float)(DS_NB - 1) ? DS_NB - 1 : max(0, (int)t);
        }
        return (int)min((f2key(v) - klo) >> sh, (uint32_t)(DS_NB - 1));     // (the clamps never bind inside the window)
    }
};

__global__ __launch_bounds__(DS_T) void dist_window_kernel(DistSrc a, int32_t *win)
{
    __shared__ uint32_t slo[DS_WAVES][DS_W], shi[DS_WAVES][DS_W], snan[DS_WAVES][DS_W];
    const int lane = threadIdx.x & (DS_W - 1), wave = threadIdx.x / DS_W;
    const long long Cp = a.Cp;
    const long long c = (long long)blockIdx.x * DS_W + lane;
    uint32_t lo = 0xffffffffu, hi = 0u, nan = 0u;
    if (c < a.C) {
        ds_rows(ds_col(a, c), a.RS, 0, a.n, wave, [&](float v) {
            const uint32_t k = f2key(v);
            const bool isn = v != v;
            nan |= isn ? 1u : 0u;
            lo = isn ? lo : min(lo, k);
            hi = isn ? hi : max(hi, k);
        });
    }
    slo[wave][lane] = lo;
    shi[wave][lane] = hi;
    snan[wave][lane] = nan;
    __syncthreads();
    if (wave == 0 && c < Cp) {
        for (int w = 1; w < DS_WAVES; ++w) {
            lo = min(lo, slo[w][lane]);
            hi = max(hi, shi[w][lane]);
            nan |= snan[w][lane];
        }
        if (c >= a.C) {                        // pad: a NaN-free constant 0.0
            lo = hi = f2key(0.0f);
            nan = 0u;
        }
        win[c] = (int32_t)(lo ^ 0x80000000u);
        win[Cp + c] = (int32_t)(~hi ^ 0x80000000u);
        win[2 * Cp + c] = nan ? 0 : 1;
    }
}

template <bool PACKED>
__global__ __launch_bounds__(DS_T) void dist_hist_kernel(DistSrc a, const int32_t *params, int32_t *hist)
{
    constexpr int WORDS = PACKED ? DS_NB / 2 : DS_NB;
    __shared__ uint32_t h[DS_NB * 32];                 // [bucket][cell & 31], cell >> 5 selects the half
    const int lane = threadIdx.x & (DS_W - 1), wave = threadIdx.x / DS_W;
    const long long Cp = a.Cp;
    const long long t0 = (long long)blockIdx.x * DS_W;
    const long long c = t0 + lane;
    DsMap m;
    m.sh = -1;
    if (c < a.C) m.load(params, Cp, c);
    const uint32_t inc = 1u << (16 * (lane >> 5));
    for (int i = threadIdx.x; i < DS_NB * 32; i += DS_T) h[i] = 0u;
    __syncthreads();
    for (long long r0 = 0; r0 < a.n; r0 += DS_CHUNK) {
        const long long r1 = min(a.n, r0 + (long long)DS_CHUNK);
        if (m.sh >= 0) {
            ds_rows(ds_col(a, c), a.RS, r0, r1, wave, [&](float v) { atomicAdd(&h[m.bucket(v) * 32 + (lane & 31)], inc); });
        }
        __syncthreads();
        // flush: thread -> (word w, cell cl): conflict-free LDS reads, writes coalesced along the cells of [W][words][Co]
        for (int i = threadIdx.x; i < WORDS * DS_W; i += DS_T) {
            const int cl = i & (DS_W - 1), w = i / DS_W;
            const long long cc = t0 + cl;
            if (cc >= Cp) continue;
            const int sh = 16 * (cl >> 5), col = cl & 31;
            uint32_t v = (h[w * 32 + col] >> sh) & 0xffffu;
            if (PACKED) v |= ((h[(w + DS_NB / 2) * 32 + col] >> sh) & 0xffffu) << 16;
            const long long r = cc / a.Co;
            int32_t *o = hist + (r * WORDS + w) * a.Co + (cc - r * a.Co);
            *o = r0 == 0 ? (int32_t)v : (int32_t)((uint32_t)*o + v);
        }
        __syncthreads();
        if (r1 < a.n) {
            for (int i = threadIdx.x; i < DS_NB * 32; i += DS_T) h[i] = 0u;
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(DS_T) void dist_collect_kernel(DistSrc a, const int32_t *params, const int32_t *want, int S,
                                                            const int32_t *cnt, const int64_t *off, float *send)
{
    extern __shared__ uint32_t lds[];
    uint32_t *bm = lds;                                // [NB / 32][cell]: is bucket b wanted?
    int32_t *wb = (int32_t *)(lds + (DS_NB / 32) * DS_W);    // [slot][cell]: its bucket
    uint32_t *pos = lds + (DS_NB / 32 + S) * DS_W;            // [slot][cell]: next free entry of its list
    const int lane = threadIdx.x & (DS_W - 1), wave = threadIdx.x / DS_W;
    const long long Cp = a.Cp;
    const long long c = (long long)blockIdx.x * DS_W + lane;
    DsMap m;
    m.sh = -1;
    if (c < a.C) m.load(params, Cp, c);
    if (wave == 0) {
        for (int j = 0; j < DS_NB / 32; ++j) bm[j * DS_W + lane] = 0u;
        for (int s = 0; s < S; ++s) {
            const int b = (m.sh >= 0) ? want[c * S + s] : -1;
            wb[s * DS_W + lane] = b;
            pos[s * DS_W + lane] = 0u;
            if (b >= 0) bm[(b >> 5) * DS_W + lane] |= 1u << (b & 31);
        }
    }
    __syncthreads();
    if (m.sh < 0) return;
    ds_rows(ds_col(a, c), a.RS, 0, a.n, wave, [&](float v) {
        const int b = m.bucket(v);
        if (!((bm[(b >> 5) * DS_W + lane] >> (b & 31)) & 1u)) return;
        int s = 0;
        while (s < S - 1 && wb[s * DS_W + lane] != b) ++s;     // (found: b is one of the cell's wanted buckets)
        const uint32_t p = atomicAdd(&pos[s * DS_W + lane], 1u);
        if (p < (uint32_t)cnt[c * S + s]) send[off[c * S + s] + p] = v;
    });
}

// one wave per owned cell: each of its slots' lists is gathered from the W segments into LDS (keys), and every element
// learns its place by counting (less, less-or-equal) over the list; the element whose place holds a wanted rank writes it
__global__ __launch_bounds__(DS_W) void dist_pick_kernel(const float *vals, const int32_t *cnt, const int64_t *off, int W,
                                                         long long Co, int S, const int32_t *slot, const int32_t *rnk, int nk,
                                                         float *out)
{
    __shared__ uint32_t keys[DS_PICK_CAP];
    const int lane = threadIdx.x;
    const long long co = blockIdx.x;
    const int ls = lane < nk ? slot[co * nk + lane] : -1;     // lane j holds rank j's slot and place
    const int lr = lane < nk ? rnk[co * nk + lane] : 0;
    int used = -1;
    for (int j = 0; j < nk; ++j) used = max(used, __shfl(ls, j));
    used = min(used, S - 1);
    for (int s = 0; s <= used; ++s) {
        int L = 0;
        for (int w = 0; w < W; ++w) L += cnt[((long long)w * Co + co) * S + s];
        if (L == 0 || L > DS_PICK_CAP) continue;
        __syncthreads();                               // the previous slot's readers are done with keys[]
        int at = 0;
        for (int w = 0; w < W; ++w) {
            const long long i = ((long long)w * Co + co) * S + s;
            const int n = cnt[i];
            const float *src = vals + off[i];
            for (int e = lane; e < n; e += DS_W) keys[at + e] = f2key(src[e]);
            at += n;
        }
        __syncthreads();
        for (int e = lane; e < L; e += DS_W) {
            const uint32_t ke = keys[e];
            int less = 0, leq = 0;
            for (int j = 0; j < L; ++j) {
                const uint32_t kj = keys[j];
                less += kj < ke;
                leq += kj <= ke;
            }
            for (int j = 0; j < nk; ++j) {
                const int sj = __builtin_amdgcn_readlane(ls, j), rj = __builtin_amdgcn_readlane(lr, j);
                if (sj == s && less <= rj && rj < leq) out[(long long)j * Co + co] = key2f(ke);
            }
        }
    }
}

bool ds_src(DistSrc &a, const float *scores, int64_t plane_stride, int64_t row_stride, int64_t planes, int64_t n, int64_t per,
            int64_t c0, int64_t C, int64_t W, int64_t Co)
{
    if (!scores || n <= 0 || per <= 0 || planes <= 0 || W <= 0 || Co <= 0 || C < 0 || c0 < 0) return false;
    if (C > W * Co || c0 + C > planes * per || (n > 1 && row_stride < per) || (planes > 1 && plane_stride < per)) return false;
    if (W > 65535 || (Co + DS_W - 1) / DS_W * W > 0x7fffffffLL) return false;
    a.s = scores;
    a.PS = plane_stride;
    a.RS = row_stride;
    a.n = n;
    a.per = per;
    a.c0 = c0;
    a.C = C;
    a.Co = Co;
    a.Cp = W * Co;
    return true;
}

// one 1024-thread workgroup per 64 cells of the padded run
unsigned ds_tiles(const DistSrc &a) { return (unsigned)((a.Cp + DS_W - 1) / DS_W); }

}  // namespace

extern "C" int pre_dist_abi_version(void) { return PRE_DIST_ABI_VERSION; }

extern "C" int pre_dist_window_f32(const float *scores, int64_t plane_stride, int64_t row_stride, int64_t planes, int64_t n,
                                   int64_t per, int64_t c0, int64_t C, int64_t W, int64_t Co, int32_t *win, void *stream)
{
    DistSrc a;
    if (!win || !ds_src(a, scores, plane_stride, row_stride, planes, n, per, c0, C, W, Co)) return PRE_E_NULL;
    hipLaunchKernelGGL(dist_window_kernel, dim3(ds_tiles(a)), dim3(DS_T), 0, as_stream(stream), a, win);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}

extern "C" int pre_dist_hist_f32(const float *scores, int64_t plane_stride, int64_t row_stride, int64_t planes, int64_t n,
                                 int64_t per, int64_t c0, int64_t C, int64_t W, int64_t Co, const int32_t *params, int packed,
                                 int32_t *hist, void *stream)
{
    DistSrc a;
    if (!params || !hist || !ds_src(a, scores, plane_stride, row_stride, planes, n, per, c0, C, W, Co)) return PRE_E_NULL;
    if (packed && n * W > 32767) return PRE_E_RANGE;             // a 16-bit half would carry into its neighbour
    if (packed)
        hipLaunchKernelGGL(dist_hist_kernel<true>, dim3(ds_tiles(a)), dim3(DS_T), 0, as_stream(stream), a, params, hist);
    else
        hipLaunchKernelGGL(dist_hist_kernel<false>, dim3(ds_tiles(a)), dim3(DS_T), 0, as_stream(stream), a, params, hist);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}

extern "C" int pre_dist_collect_f32(const float *scores, int64_t plane_stride, int64_t row_stride, int64_t planes, int64_t n,
                                    int64_t per, int64_t c0, int64_t C, int64_t W, int64_t Co, const int32_t *params,
                                    const int32_t *want, int S, const int32_t *cnt, const int64_t *off, float *send, void *stream)
{
    DistSrc a;
    if (!params || !want || !cnt || !off || !ds_src(a, scores, plane_stride, row_stride, planes, n, per, c0, C, W, Co))
        return PRE_E_NULL;
    if (S < 1 || S > PRE_DIST_MAX_SLOTS) return PRE_E_RANGE;
    if (!send) send = (float *)off;          // (nothing to send: no element is wanted, the kernel writes nothing)
    const size_t lds = (size_t)(DS_NB / 32 + 2 * S) * DS_W * sizeof(uint32_t);
    hipLaunchKernelGGL(dist_collect_kernel, dim3(ds_tiles(a)), dim3(DS_T), lds, as_stream(stream), a, params, want, S, cnt, off,
                       send);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}

extern "C" int pre_dist_pick_f32(const float *vals, const int32_t *cnt, const int64_t *off, int64_t W, int64_t Co, int S,
                                 const int32_t *slot, const int32_t *rnk, int nk, float *out, void *stream)
{
    if (!cnt || !off || !slot || !rnk || !out || W <= 0 || W > PRE_DIST_MAX_SLOTS * 1024 || Co <= 0) return PRE_E_NULL;
    if (S < 1 || S > PRE_DIST_MAX_SLOTS || nk < 1 || nk > PRE_DIST_MAX_SLOTS || Co > 0x7fffffffLL) return PRE_E_RANGE;
    if (!vals) vals = (const float *)off;    // (nothing received: every list is empty, nothing is read)
    hipLaunchKernelGGL(dist_pick_kernel, dim3((unsigned)Co), dim3(DS_W), 0, as_stream(stream), vals, cnt, off, (int)W, (long long)Co,
                       S, slot, rnk, nk, out);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}
