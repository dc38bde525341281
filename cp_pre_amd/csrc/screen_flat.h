// screen_flat.h - the merged-row march of the calibrated-set screen for Nt-fastest fields (screen_flat_kernel), its geometry,
// launchers, host checks and the relabelling of the stars, shared by screen_flat.hip (libcp_pre_screenflat.so) and
// screen_jorek.hip (libcp_pre_screenjorek.so).  What the march does is told at the head of screen_flat.hip.
#pragma once
#include "screen_plane.h"
#include "../../include/cp_pre_screenflat.h"

namespace {

constexpr int FLAT_NW = FLAT_NT / 64;        // most waves per workgroup

// Kernel axes: T = the marched axis (logical Nx), X = logical Ny, Y = logical Nt; a plane is one row of X * Y cells.
struct FGeom {
    const float *f[MAXF];
    long long sB[MAXF], sT[MAXF];        // sample and marched-plane strides (elements)
    const float *mod;                    // nullptr: m == 1
    long long mT;                        // its marched-plane stride
    const float *q;                      // device, nk levels
    unsigned int *score;                 // [B]
    unsigned int *count;                 // [nk][cld]
    long long cld;
    int B, T, X, Y;
    int tSeg, nTSeg, nCh;
    int cT, cX, cY, nk;                  // cells per side left out of the counted region, on the kernel's axes
};

// Waves per SIMD the register allocator leaves room for.  The forward pass caps NS momentum in this layout at 128
// registers (NSMomentum::MIN_WAVES, a few dwords spilled); with the epilogue's live values that cap would mean scratch inside
// the plane loop, and an instantiation with scratch is not built: every functor gets the whole register file here.
template <class Fn> struct ScreenMinWaves { static constexpr int value = 1; };

template <class Fn, class Sets = ScalarSets>
__global__ void __launch_bounds__(FLAT_NT, ScreenMinWaves<Fn>::value)
screen_flat_kernel(const FGeom g, const typename Fn::Params prm, const Sets sets)
{
    constexpr int F = Fn::F;
    constexpr bool CELLS = Sets::CELLS;
    constexpr bool STATS = IsStats<Sets>::value;   // (per-sample statistics: no levels, no modulation, screen_plane.h)
    constexpr int LB = CellsBatch<Fn>::value;      // (per-cell sets: level quads held across the functor ...
    constexpr int LL = CellsLate<Fn>::value;       //  ... and per batch fetched after it)
    static_assert(LB >= 1 && LB <= NKMAX && (LB == NKMAX || (LL >= 1 && (NKMAX - LB) % LL == 0)), "whole batches");
    using SX = Staged<Fn>;
    constexpr bool ANY = SX::count > 0;
    static_assert(256 >= NKMAX + 1, "one thread per result in the combine step (the narrowest chunk has 256 threads)");
    __shared__ float4 lds[2][SX::FX][ANY ? FLAT_NT + 2 * FLAT_H : 1];
    __shared__ unsigned int red[NKMAX + 1][FLAT_NW];
    const int q = threadIdx.x;
    unsigned Lb = xcd_remap(blockIdx.x, gridDim.x);
    [[maybe_unused]] const unsigned slot = Lb;     // (statistics: this workgroup's slot of the workspace)
    // per-cell sets: a group of CELLS_G samples is the fastest index, so the workgroups an XCD runs together (contiguous in
    // Lb) read the same level quads and find them in its L2; the last group is partial when B % CELLS_G != 0
    const int bl = CELLS ? Lb % CELLS_G : 0;
    if constexpr (CELLS) Lb /= CELLS_G;
    const int ch = Lb % g.nCh; Lb /= g.nCh;
    const int ts = Lb % g.nTSeg;
    const int b = CELLS ? (Lb / g.nTSeg) * CELLS_G + bl : Lb / g.nTSeg;
    if constexpr (CELLS)
        if (b >= g.B) return;                      // (workgroup-uniform: no such sample in the last group)
    const int Ty = g.Y, L = g.X * g.Y;
    const int NT = blockDim.x;                     // threads per chunk, chosen by the host (the LDS image is sized for 512)

    // the planes this workgroup evaluates: its segment, less the planes outside the counted region
    const int t0 = max(ts * g.tSeg, g.cT);
    const int t1 = min(min(ts * g.tSeg + g.tSeg, g.T), g.T - g.cT);
    if (t0 >= t1) {                                // (workgroup-uniform: nothing of this segment is counted)
        if constexpr (STATS)
            if (q == 0) stats_store(sets, slot, 0.0, 0.0, 0.0);                 // (the second launch reads every slot)
        return;
    }

    const int m0 = ch * NT * 4, m = m0 + 4 * q;
    const bool inb = m < L;                        // (whole quads only: L % 4 == 0, checked by the host)

    // halo duty (staged fields): the first / last HQ threads fetch one quad left / right of the chunk, HQ = the quads an
    // x-neighbour (Ty cells away) can reach into.  The LDS image keeps room for FLAT_H quads per side.
    const int HQ = min(FLAT_H, (Ty + 3) >> 2);
    const bool hl = q < HQ, hr = q >= NT - HQ;
    const int hm = hl ? m0 - 4 * (HQ - q) : m0 + 4 * NT + 4 * (q - (NT - HQ));
    const bool hok = (hl || hr) && hm >= 0 && hm < L;
    const int hslot = hl ? FLAT_H - HQ + q : FLAT_H + NT + (q - (NT - HQ));

    // per cell of my quad: does it have a y- / y+ neighbour inside its own x row, and is it counted - (x, y) = (m / Ty,
    // m % Ty) recovered per element, because a quad straddles a row end when Ty % 4 != 0
    bool lok[4], rok[4], keep[4];
    {
        int ph = m % Ty, xr = m / Ty;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lok[j] = ph != 0;
            rok[j] = ph != Ty - 1;
            keep[j] = inb && xr >= g.cX && xr < g.X - g.cX && ph >= g.cY && ph < Ty - g.cY;
            if (++ph == Ty) { ph = 0; ++xr; }
        }
    }
    const bool anykeep = keep[0] || keep[1] || keep[2] || keep[3];
    // edge duty (unstaged fields): a wave's first lane fetches the cell before its quad, its last lane the cell after -
    // if that cell is a y-neighbour at all (same x row; the row's last cell has rok == false, so nothing beyond L is read)
    const bool ledge = (q & 63) == 0, redge = (q & 63) == 63;
    const bool eload = inb && (ledge ? lok[0] : (redge && rok[3]));

    // a plane of a field of this sample = a wave-uniform buffer descriptor; the thread's own quad and its halo quad are
    // two 32-bit byte offsets shared by every field and by the modulation (one in-plane layout)
    const unsigned int voff = (unsigned int)m * 4u, hoff = (unsigned int)hm * 4u;       // (hm < 0: never loaded)
    const unsigned int eoff = ledge ? voff - 4u : voff + 16u;                           // (never loaded where it would be outside)
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    auto rsrc = [&](int i, int t) __attribute__((always_inline)) {
        const float *p = g.f[i] + ((long long)b * g.sB[i] + (long long)t * g.sT[i]);
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, -1, 0x00020000);
    };
    auto quad = [&](int i, int t, unsigned int off) __attribute__((always_inline)) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc(i, t), (int)off, 0, 0);
        return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    };

    auto load_own = [&](int t, float4(&dst)[F]) __attribute__((always_inline)) {
        const bool ok = inb && (t >= 0) && (t < g.T);
#pragma unroll
        for (int i = 0; i < F; ++i) {
            if (ok) dst[i] = quad(i, t, voff);
            else dst[i] = f4(0.f);
        }
    };
    auto load_halo = [&](int t, FlatHalo<F> &h) __attribute__((always_inline)) {
        const bool okt = (t >= 0) && (t < g.T);
#pragma unroll
        for (int i = 0; i < F; ++i) {
            if (SX::has(i)) {
                h.e[i] = 0.f;
                if (hok && okt) h.q[i] = quad(i, t, hoff);
                else h.q[i] = f4(0.f);
            } else {
                h.q[i] = f4(0.f);
                h.e[i] = (eload && okt) ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc(i, t), (int)eoff, 0, 0)) : 0.f;
            }
        }
    };
    // the modulation quad of plane t: only by threads with a counted cell and only for planes of this segment (a rim
    // cell that shares its quad with counted ones is masked by the select)
    auto load_mod = [&](int t, float4 &dst) __attribute__((always_inline)) {
        if constexpr (STATS) {
            dst = f4(1.0f);                        // (no modulation under this policy: no registers for it either)
        } else if (g.mod && anykeep && t < t1) {
            const float *p = g.mod + (long long)t * g.mT;
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(
                __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, -1, 0x00020000), (int)voff, 0, 0);
            dst = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
        } else {
            dst = f4(1.0f);
        }
    };

    // per-cell sets: the quads of levels [k0, k0 + N) at plane t into dst[N], loaded like the modulation - only by threads
    // with a counted cell, and t is always a plane of this segment.  ql: the first batch, held across the functor (load_lev);
    // qm: a later batch, fetched after it (load_late)
    [[maybe_unused]] float4 ql[CELLS ? LB : 1], qm[CELLS && LB < NKMAX && LL != LB ? LL : 1];
    [[maybe_unused]] auto load_quads = [&](int t, int k0, auto &dst) __attribute__((always_inline)) {
        if constexpr (CELLS) {
            constexpr int N = std::extent<std::remove_reference_t<decltype(dst)>>::value;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                if (anykeep && k0 + k < g.nk) {
                    const float *p = g.q + ((long long)(k0 + k) * sets.qK + (long long)t * sets.qT);
                    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(
                        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, -1, 0x00020000), (int)voff, 0, 0);
                    dst[k] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
                } else {
                    dst[k] = f4(0.f);
                }
            }
        }
    };
    [[maybe_unused]] auto load_lev = [&](int t) __attribute__((always_inline)) {
        load_quads(t, 0, ql);
    };
    [[maybe_unused]] auto load_late = [&](int t, int k0) __attribute__((always_inline)) {
        load_quads(t, k0, qm);
    };

    // the levels: wave-uniform, read once (per-cell sets: a quad per level and plane, load_lev)
    float qk[NKMAX];
    unsigned int cnt[NKMAX];
#pragma unroll
    for (int k = 0; k < NKMAX; ++k) {
        if constexpr (CELLS || STATS) qk[k] = 0.f;
        else qk[k] = k < g.nk ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g.q[k]))) : 0.f;
        cnt[k] = 0;
    }
    float smax = 0.f, sthr = 0.f;
    bool snan = false;
    [[maybe_unused]] double sacc[3] = {0.0, 0.0, 0.0};      // (statistics: sum r, sum |r|, sum r^2 of this thread's cells)

    auto step = [&](int t, float4(&P)[F], float4(&C)[F], float4(&N)[F], float4(&D)[F], FlatHalo<F> &hc, FlatHalo<F> &hn,
                    float4 &mc, float4 &mn) __attribute__((always_inline)) {
        const int bi = (t - t0) & 1;
        // per-cell sets: this plane's first LB level quads go out BEFORE the field loads below, so the wait for them at the
        // end of the plane (vmcnt retires in issue order) leaves the loads of the coming planes in flight
        load_lev(t);
#pragma unroll
        for (int i = 0; i < F; ++i) {
            if (!SX::has(i)) continue;
            const int k = SX::slot(i);
            lds[bi][k][FLAT_H + q] = C[i];
            if (hl || hr) lds[bi][k][hslot] = hc.q[i];
        }
        // issue order = order of first use: the halo of t+1 is staged first at the next plane, the own cells of t+2 are read
        // there as t+1, the modulation of t+1 after that plane's functor
        load_halo(t + 1, hn);
        load_own(t + 2, D);
        load_mod(t + 1, mn);
        if constexpr (ANY) lds_barrier();

        Nbr n[F];
#pragma unroll
        for (int i = 0; i < F; ++i) {
            n[i].c = C[i];
            n[i].tm = P[i];
            n[i].tp = N[i];
            float lft, rgt;
            if (SX::has(i)) {
                const int k = SX::slot(i);
                const float *row = reinterpret_cast<const float *>(&lds[bi][k][0]) + 4 * (FLAT_H + q);      // my first cell
                if ((Ty & 1) == 0) {                     // Ty = 10, 30, 50 (T_out of the reference scripts): 8-byte aligned pairs
                    const float2 a = *reinterpret_cast<const float2 *>(row - Ty), b2 = *reinterpret_cast<const float2 *>(row + 2 - Ty);
                    const float2 c = *reinterpret_cast<const float2 *>(row + Ty), d = *reinterpret_cast<const float2 *>(row + 2 + Ty);
                    n[i].xm = make_float4(a.x, a.y, b2.x, b2.y);
                    n[i].xp = make_float4(c.x, c.y, d.x, d.y);
                } else {
                    n[i].xm = make_float4(row[-Ty], row[1 - Ty], row[2 - Ty], row[3 - Ty]);
                    n[i].xp = make_float4(row[Ty], row[Ty + 1], row[Ty + 2], row[Ty + 3]);
                }
                lft = row[-1];
                rgt = row[4];
            } else {
                n[i].xm = n[i].xp = f4(__builtin_nanf(""));      // never read by the functor (or the result says so)
                lft = lane_below(C[i].w);
                rgt = lane_above(C[i].x);
                lft = ledge ? hc.e[i] : lft;
                rgt = redge ? hc.e[i] : rgt;
            }
            n[i].ym = make_float4(lok[0] ? lft : 0.f, lok[1] ? C[i].x : 0.f, lok[2] ? C[i].y : 0.f, lok[3] ? C[i].z : 0.f);
            n[i].yp = make_float4(rok[0] ? C[i].y : 0.f, rok[1] ? C[i].z : 0.f, rok[2] ? C[i].w : 0.f, rok[3] ? rgt : 0.f);
        }
        const float4 r = Fn::eval(n, prm);
        if constexpr (STATS) {
            stats_plane(r, keep, sacc, smax, snan);
        } else if constexpr (!CELLS) {
            screen_plane(r, mc, keep, g.nk, qk, cnt, smax, sthr, snan);
        } else if constexpr (LB == NKMAX) {
            screen_plane_cells(r, mc, keep, g.nk, ql, cnt, smax, sthr, snan);
        } else {
            float ac[4], sv[4];
            screen_plane_score(r, mc, keep, ac, sv, smax, sthr, snan);
            if constexpr (LL == LB) {
                // later batches of the first one's size reuse its registers: in a second array they cost the six-field
                // functors of screen_cells.hip a register
#pragma unroll
                for (int k0 = 0; k0 < NKMAX; k0 += LB) {
                    if (k0 >= g.nk) break;                 // (wave-uniform)
                    if (k0 > 0) load_quads(t, k0, ql);
                    screen_plane_count<LB>(ac, sv, k0, g.nk, ql, cnt);
                }
            } else {
                screen_plane_count<LB>(ac, sv, 0, g.nk, ql, cnt);
#pragma unroll
                for (int k0 = LB; k0 < NKMAX; k0 += LL) {
                    if (k0 >= g.nk) break;                 // (wave-uniform)
                    load_late(t, k0);
                    screen_plane_count<LL>(ac, sv, k0, g.nk, qm, cnt);
                }
            }
        }
    };

    float4 w0[F], w1[F], w2[F], w3[F], md0, md1;
    FlatHalo<F> h0, h1;
    load_own(t0 - 1, w0);
    load_own(t0, w1);
    load_own(t0 + 1, w2);
    load_halo(t0, h0);
    load_mod(t0, md0);
    for (int t = t0; t < t1; t += 4) {
        step(t, w0, w1, w2, w3, h0, h1, md0, md1);
        if (t + 1 >= t1) break;
        step(t + 1, w1, w2, w3, w0, h1, h0, md1, md0);
        if (t + 2 >= t1) break;
        step(t + 2, w2, w3, w0, w1, h0, h1, md0, md1);
        if (t + 3 >= t1) break;
        step(t + 3, w3, w0, w1, w2, h1, h0, md1, md0);
    }

    // combine: the waves of the workgroup through LDS, then one integer atomic per result for this sample.  Non-negative
    // floats order like their bit patterns and the NaN pattern lies above +inf: the unsigned maximum is the float maximum
    // with NaN sticky, across workgroups and across calls.
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) smax = fmaxf(smax, __shfl_xor(smax, o));
    const unsigned int ubits = __ballot(snan) ? 0x7fc00000u : __float_as_uint(smax);
    const int wv = q >> 6, nw = NT >> 6;
    if constexpr (STATS) {
        // statistics: the maximum as below; the sums by shuffles, then LDS in wave order, then ONE slot of the workspace
        __shared__ double dred[3][FLAT_NW];
        stats_wave(sacc);
        if ((q & 63) == 0) {
            red[0][wv] = ubits;
#pragma unroll
            for (int j = 0; j < 3; ++j) dred[j][wv] = sacc[j];
        }
        __syncthreads();
        if (q == 0) {
            unsigned int v = 0;
            double s[3] = {0.0, 0.0, 0.0};
            for (int w = 0; w < nw; ++w) {
                v = max(v, red[0][w]);
#pragma unroll
                for (int j = 0; j < 3; ++j) s[j] += dred[j][w];
            }
            if (v) atomicMax(g.score + b, v);
            stats_store(sets, slot, s[0], s[1], s[2]);
        }
        return;
    }
    if ((q & 63) == 0) {
        red[0][wv] = ubits;
#pragma unroll
        for (int k = 0; k < NKMAX; ++k) red[1 + k][wv] = cnt[k];
    }
    __syncthreads();
    if (q <= g.nk) {
        unsigned int v = 0;
        for (int w = 0; w < nw; ++w) v = q == 0 ? max(v, red[0][w]) : v + red[q][w];
        if (v) {
            if (q == 0) atomicMax(g.score + b, v);
            else atomicAdd(g.count + (long long)(q - 1) * g.cld + b, v);
        }
    }
}

// ------------------------------------------------------------------ host side
template <class Fn, class Sets = ScalarSets>
int launch_screen_flat(FGeom &g, const typename Fn::Params &prm, hipStream_t st, const Sets &sets = Sets())
{
    static_assert(2 * Staged<Fn>::FX * (FLAT_NT + 2 * FLAT_H) * 16 + (NKMAX + 1) * FLAT_NW * 4 <= 160 * 1024, "chunk does not fit the 160 KiB LDS");
    static_assert(FLAT_NOLDS_NT <= FLAT_NT, "the kernel's launch bound and its reduction buffer are sized for FLAT_NT threads");
    const long long quads = (long long)g.X * g.Y / 4;
    const int nt = flat_chunk(quads, g.Y, Staged<Fn>::count > 0);
    g.nCh = (int)((quads + nt - 1) / nt);
    static std::atomic<int> per_cu[FLAT_NT / 64 + 1] = {};         // (by chunk width)
    unsigned grid;
    // (per-cell sets: the grid covers whole groups of CELLS_G samples)
    const long long nb = Sets::CELLS ? ((long long)g.B + CELLS_G - 1) / CELLS_G * CELLS_G : g.B;
    const int rc = flat_split(screen_flat_kernel<Fn, Sets>, nt, per_cu, g, nb * g.nCh, g.T, &grid);
    if (rc) return rc;
    if constexpr (IsStats<Sets>::value)
        if (!stats_room(sets, grid)) return PRE_E_NULL;                    // (never with the length the query entry gives)
    hipLaunchKernelGGL((screen_flat_kernel<Fn, Sets>), dim3(grid), dim3(nt), 0, st, g, prm, sets);
    PRE_LAUNCH_CHECK();
    if constexpr (IsStats<Sets>::value) return stats_finish(sets, g.B, (long long)grid / g.B, st);
    return PRE_OK;
}

// statistics: an upper bound of the workgroups per sample of any launch_screen_flat on the logical (T, X, Y), from the shape
// alone - chunks no narrower than 256 quads (flat_chunk) and marches of Nx no shorter than min(X, 8) planes (pick_tseg)
inline long long stats_slots_flat(long long T, long long X, long long Y)
{
    const long long quads = (Y * T + 3) / 4;
    return ((quads + 255) / 256) * ((X + 7) / 8);
}

// the tap structures an Nt-fastest view runs (relabeled_mode: the reference's construction, the y-fixed one, the general star)
template <template <int> class FnT, class P, class Sets = ScalarSets>
int launch_screen_flat_mode(int mode, FGeom &g, const P &prm, hipStream_t st, const Sets &sets = Sets())
{
    if (mode == 3) return launch_screen_flat<FnT<3>>(g, prm, st, sets);
    if (mode == 4) return launch_screen_flat<FnT<4>>(g, prm, st, sets);
    return launch_screen_flat<FnT<2>>(g, prm, st, sets);
}

// Null / empty / range / layout checks of everything an entry hands to the kernel, and the geometry on the kernel's axes.
// Shapes and crops come in on the caller's logical [B,T,X,Y].
int prepare_flat(FGeom &g, const pre_field_t *const *fs, int nf, const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X,
                 int64_t Y, int flags)
{
    const int rc = screen_args(fs, nf, s, NKMAX, B, T, X, Y, 0);
    if (rc) return rc;
    if (flags & ~PRE_FLAG_INTERIOR_T) return PRE_E_UNSUPPORTED;                          // (PRE_FLAG_HALO_X among them)
    // the layout pre_residual_* takes its flat form on after relabelling: T contiguous, Y's stride == T, a short T
    if (T >= FLAT_MAX_Y || Y <= 1 || (Y * T) % 4 != 0) return PRE_E_UNSUPPORTED;
    for (int i = 0; i < nf; ++i)
        if (fs[i]->sT != 1 || fs[i]->sY != T) return PRE_E_UNSUPPORTED;
    if (s->modulation && (s->mT != 1 || s->mY != T)) return PRE_E_UNSUPPORTED;
    if (Y * T >= (1LL << 30)) return PRE_E_SHAPE;                  // a thread's place in a plane is a 32-bit byte offset
    for (int i = 0; i < MAXF; ++i) {
        const bool on = i < nf;
        g.f[i] = on ? fs[i]->ptr : nullptr;
        g.sB[i] = on ? fs[i]->sB : 0; g.sT[i] = on ? fs[i]->sX : 0;
    }
    g.mod = s->modulation; g.mT = s->mX;
    g.q = s->q; g.score = s->score; g.count = s->count; g.cld = s->count_ld;
    g.B = (int)B; g.T = (int)X; g.X = (int)Y; g.Y = (int)T;
    g.cT = s->cx; g.cX = s->cy; g.cY = (flags & PRE_FLAG_INTERIOR_T) ? (s->ct > 1 ? s->ct : 1) : s->ct;
    g.nk = s->nk;
    return PRE_OK;
}

// prepare()'s relabelling of the star weights for kernel axes (X, Y, T): the logical x-taps sit on the marched axis, the
// y-taps on the kernel's x, the t-taps on its y
void relabel_stars(Star *const *stars, int n)
{
    for (int k = 0; k < n; ++k) {
        const Star o = *stars[k];
        stars[k]->tm = o.xm; stars[k]->tp = o.xp;
        stars[k]->xm = o.ym; stars[k]->xp = o.yp;
        stars[k]->ym = o.tm; stars[k]->yp = o.tp;
    }
}

}  // namespace
