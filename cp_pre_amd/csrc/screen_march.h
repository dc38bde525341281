// screen_march.h - the march of the calibrated-set screen for Ny-fastest fields (screen_march_kernel), its geometry, launchers
// and host checks, shared by screen_march.hip (libcp_pre_screen.so) and screen_jorek.hip (libcp_pre_screenjorek.so).  What the
// march does is told at the head of screen_march.hip.
#pragma once
#include "screen_plane.h"

namespace {

struct SGeom {
    const float *f[MAXF];
    long long sB[MAXF], sT[MAXF], sX[MAXF];
    const float *mod;            // nullptr: m == 1
    long long mT, mX;
    const float *q;              // device, nk levels
    unsigned int *score;         // [B]
    unsigned int *count;         // [nk][cld]
    long long cld;
    int B, T, X, Y;
    int tSeg, nTSeg, nXT, nYT;
    int flags;
    int tfree;                   // no operator has a tap along the marched axis: a segment loads its own planes only
    int ct, cx, cy, nk;
};

// Waves per SIMD the register allocator must leave room for: MinWaves<Fn>, and for the BC form under the level policies what
// the functor asks for it (Fn::SCREEN_BC_MIN_WAVES, optional).  The statistics policy never takes that request: its fp64
// accumulators sit next to the functor, and where a functor needs the request it costs scratch there
// (profiles/screenbc/resources.txt).
template <class Fn, class = void> struct ScreenBCMinWaves { static constexpr int value = MinWaves<Fn>::value; };
template <class Fn> struct ScreenBCMinWaves<Fn, std::void_t<decltype(Fn::SCREEN_BC_MIN_WAVES)>> {
    static constexpr int value = Fn::SCREEN_BC_MIN_WAVES;
};
template <class Fn, class Sets, bool BC> struct MarchMinWaves {
    static constexpr int value = (BC && !IsStats<Sets>::value) ? ScreenBCMinWaves<Fn>::value : MinWaves<Fn>::value;
};

// BC: boundary conditions on the x-y rim, as march_kernel<Fn, NR, TYQ, BC> of star_march.h takes them (BCInfo, host_checks.h):
// the halo row beyond the grid is the mapped row or the side's constant, the row x == X of a partial last tile is a ghost row
// that loads its mapped row and never counts, the last quad of a row keeps a second edge scalar (Halo::yr).  What is counted,
// the modulation, the levels, the accumulators and the combine step do not know of it.
template <class Fn, int NR, int TYQ, class Sets = ScalarSets, bool BC = false>
__global__ void __launch_bounds__(NR *TYQ, (MarchMinWaves<Fn, Sets, BC>::value))
screen_march_kernel(const SGeom g, const typename Fn::Params prm, const Sets sets,
                    const typename std::conditional<BC, BCInfo, NoBC>::type bc)
{
    constexpr int F = Fn::F;
    constexpr bool CELLS = Sets::CELLS;
    constexpr bool STATS = IsStats<Sets>::value;   // (per-sample statistics: no levels, no modulation, screen_plane.h)
    constexpr bool LACC = STATS && StatsLdsAcc<Fn>::value;      // (... its accumulators in LDS between planes)
    constexpr int LB = CellsBatch<Fn>::value;      // (per-cell sets: level quads held across the functor ...
    constexpr int LL = CellsLate<Fn>::value;       //  ... and per batch fetched after it)
    static_assert(LB >= 1 && LB <= NKMAX && (LB == NKMAX || (LL >= 1 && (NKMAX - LB) % LL == 0)), "whole batches");
    using SX = Staged<Fn>;
    constexpr int NW = NR * TYQ / 64;
    static_assert(NR >= 8 && (4 * TYQ) % 64 == 0 && (NR * TYQ) % 64 == 0, "the two halo rows are fetched by the first 8*TYQ threads, a wave per 64 floats");
    static_assert(NR * TYQ >= NKMAX + 1, "one thread per result in the combine step");
    __shared__ float4 lds[2][SX::FX][NR + 2][TYQ];
    __shared__ unsigned int red[NKMAX + 1][NW];

    const int q = threadIdx.x, ty = threadIdx.y;
    unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    [[maybe_unused]] const unsigned slot = L;      // (statistics: this workgroup's slot of the workspace)
    // per-cell sets: a group of CELLS_G samples is the fastest index, so the workgroups an XCD runs together (contiguous in
    // L) read the same level quads and find them in its L2; the last group is partial when B % CELLS_G != 0
    const int bl = CELLS ? L % CELLS_G : 0;
    if constexpr (CELLS) L /= CELLS_G;
    const int yt = L % g.nYT; L /= g.nYT;
    const int xt = L % g.nXT; L /= g.nXT;
    const int ts = L % g.nTSeg;
    const int b = CELLS ? (L / g.nTSeg) * CELLS_G + bl : L / g.nTSeg;
    if constexpr (CELLS)
        if (b >= g.B) return;                      // (workgroup-uniform: no such sample in the last group)

    // the planes this workgroup evaluates: its segment, less the planes outside the counted region
    const int tc = (g.flags & PRE_FLAG_INTERIOR_T) ? max(g.ct, 1) : g.ct;
    const int t0 = max(ts * g.tSeg, tc);
    const int t1 = min(min(ts * g.tSeg + g.tSeg, g.T), g.T - tc);
    if (t0 >= t1) {                                // (workgroup-uniform: nothing of this segment is counted)
        if constexpr (STATS)
            if (q == 0 && ty == 0) stats_store(sets, slot, 0.0, 0.0, 0.0);      // (the second launch reads every slot)
        return;
    }

    const int x = xt * NR + ty, y = (yt * TYQ + q) * 4;
    const bool inb = (x < g.X) && (y < g.Y);       // (whole quads only: Y % 4 == 0, checked by the host)
    // PRE_FLAG_HALO_X, partial last tile: row X is real data and the x+ neighbour of row X-1 (loaded, never counted)
    bool ldown = inb || ((g.flags & PRE_FLAG_HALO_X) && x == g.X && y < g.Y);
    // BC (never with PRE_FLAG_HALO_X): that row is a ghost row, which loads the row the side maps to, or holds its constant
    // (a side's constant is a kernel argument, hence a scalar register: a thread keeps the predicate that it applies - gconst,
    // hclo / hchi, lconst, rconst below - and selects the scalar after the load, where a per-thread fill value would be one
    // more vector register each, live across the plane loop)
    int xl = x;
    [[maybe_unused]] bool gconst = false;
    if constexpr (BC) {
        ldown = inb;
        if (x == g.X && y < g.Y) { xl = bc.xhi; ldown = bc.xhi >= 0; gconst = bc.xhi < 0; }
    }
    const bool kx = inb && x >= g.cx && x < g.X - g.cx;
    const bool keep[4] = {kx && y >= g.cy && y < g.Y - g.cy, kx && y + 1 >= g.cy && y + 1 < g.Y - g.cy,
                          kx && y + 2 >= g.cy && y + 2 < g.Y - g.cy, kx && y + 3 >= g.cy && y + 3 < g.Y - g.cy};
    const bool anykeep = keep[0] || keep[1] || keep[2] || keep[3];

    // halo-row duty: the workgroup's first 4*TYQ threads fetch the row above the tile, the next 4*TYQ the row below, one
    // float each; functors of five or more fields keep march_kernel's float4 form (a thread of the tile's first / last row
    // fetches its own quad of the row beyond)
    constexpr bool COOP = F <= MARCH_COOP_MAXF;
    const int hl = ty * TYQ + q;
    const bool hduty = COOP ? hl < 8 * TYQ : (ty == 0 || ty == NR - 1), hbot = COOP ? hl >= 4 * TYQ : ty == NR - 1;
    const int hcol = COOP ? hl & (4 * TYQ - 1) : 4 * q;
    const int hy = yt * (4 * TYQ) + hcol;
    int hx = hbot ? xt * NR + NR : xt * NR - 1;
    const bool halox = (g.flags & PRE_FLAG_HALO_X) != 0;
    bool hrow = hduty && (halox ? (hx >= -1 && hx <= g.X) : (hx >= 0 && hx < g.X)) && (hy < g.Y);
    const int hslot = hbot ? NR + 1 : 0;
    // y-halo duty: ONE edge scalar per lane (y- for a wave's first lane, y+ for a wave's / tile's last lane)
    const bool ledge = ((q & 63) == 0);
    bool redge = ((q & 63) == 63) || (q == TYQ - 1);
    bool eload = ledge ? (inb && y > 0) : (redge && inb && y + 4 < g.Y);
    int eoff4 = 4 * (ledge ? -1 : 4);
    // BC: the row beyond the grid and the cells beyond a row's ends by BCInfo, as march_kernel; `ye` is then the y- scalar of
    // every lane that needs one and `yr` the y+ scalar (the last quad of a row is a right edge wherever it lies in its wave)
    [[maybe_unused]] bool hclo = false, hchi = false, lconst = false, rconst = false, rload = false;
    [[maybe_unused]] int yroff4 = 16;
    if constexpr (BC) {
        if (hduty && hy < g.Y && (hx == -1 || hx == g.X)) {
            const int m = hx < 0 ? bc.xlo : bc.xhi;
            hclo = hx < 0 && m < 0;
            hchi = hx >= 0 && m < 0;
            hrow = m >= 0;
            hx = m >= 0 ? m : 0;
        }
        eload = ledge && inb && y > 0;
        rload = redge && inb && y + 4 < g.Y;
        if (inb && y == 0) { eload = bc.ylo >= 0; eoff4 = 4 * bc.ylo; lconst = bc.ylo < 0; }
        if (inb && y + 4 >= g.Y) { redge = true; rload = bc.yhi >= 0; yroff4 = 4 * (bc.yhi - y); rconst = bc.yhi < 0; }
    }

    // Addresses as in march_kernel: a plane of a field of this sample is a wave-uniform buffer descriptor based one row
    // BEFORE row 0, a thread's place in it a 32-bit byte offset (the host has checked that every offset fits)
    unsigned int voff[F], hoff[F];
#pragma unroll
    for (int i = 0; i < F; ++i) {
        voff[i] = (unsigned int)(((long long)(xl + 1) * g.sX[i] + y) * 4);
        hoff[i] = (unsigned int)(((long long)(hx + 1) * g.sX[i] + hy) * 4);
    }
    const unsigned int moff = (unsigned int)(((long long)x * g.mX + y) * 4);
    const int tlo = g.tfree ? t0 : 0, thi = g.tfree ? t1 : g.T;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    auto plane = [&](int i, int t) __attribute__((always_inline)) {
        const float *p = g.f[i] + ((long long)b * g.sB[i] - g.sX[i] + (long long)t * g.sT[i]);
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, -1, 0x00020000);
    };

    auto load_own = [&](int t, float4(&dst)[F]) __attribute__((always_inline)) {
        const bool ok = ldown && (t >= tlo) && (t < thi);
#pragma unroll
        for (int i = 0; i < F; ++i) {
            if (ok) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(plane(i, t), (int)voff[i], 0, 0);
                dst[i] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
            } else {
                dst[i] = f4(0.f);
            }
            if constexpr (BC)
                if (gconst) dst[i] = f4(bc.vxhi);
        }
    };
    auto load_halo = [&](int t, Halo<F, BC, COOP> &h) __attribute__((always_inline)) {
        const bool okt = (t >= tlo) && (t < thi);
#pragma unroll
        for (int i = 0; i < F; ++i) {
            if (!SX::has(i)) {
                if constexpr (COOP) h.row[i] = 0.f; else h.row[i] = f4(0.f);
            } else if constexpr (COOP) {
                h.row[i] = (hrow && okt) ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(plane(i, t), (int)hoff[i], 0, 0)) : 0.f;
                if constexpr (BC) {
                    if (hclo) h.row[i] = bc.vxlo;
                    if (hchi) h.row[i] = bc.vxhi;
                }
            } else if (hrow && okt) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(plane(i, t), (int)hoff[i], 0, 0);
                h.row[i] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
            } else {
                h.row[i] = f4(0.f);
                if constexpr (BC) {
                    if (hclo) h.row[i] = f4(bc.vxlo);
                    if (hchi) h.row[i] = f4(bc.vxhi);
                }
            }
            h.ye[i] = (eload && okt) ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(plane(i, t), (int)voff[i] + eoff4, 0, 0)) : 0.f;
            if constexpr (BC) {
                h.yr[i] = (rload && okt) ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(plane(i, t), (int)voff[i] + yroff4, 0, 0)) : 0.f;
                if (lconst) h.ye[i] = bc.vylo;
                if (rconst) h.yr[i] = bc.vyhi;
            }
        }
    };
    // the modulation quad of plane t: only by threads with a counted cell and only for planes of this segment (its rim
    // is never touched along t and x; along y a rim cell shares its quad with counted ones and is masked by the select)
    auto load_mod = [&](int t, float4 &dst) __attribute__((always_inline)) {
        if constexpr (STATS) {
            dst = f4(1.0f);                        // (no modulation under this policy: no registers for it either)
        } else if (g.mod && anykeep && t < t1) {
            const float *p = g.mod + (long long)t * g.mT;
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(
                __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, -1, 0x00020000), (int)moff, 0, 0);
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
                        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, -1, 0x00020000),
                        (int)(unsigned int)(((long long)x * sets.qX + y) * 4), 0, 0);
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
    [[maybe_unused]] double *lacc = nullptr;                // (... or this thread's slot of them in LDS: lacc[j * NR * TYQ])
    if constexpr (LACC) {
        __shared__ double accs[3][NR * TYQ];
        lacc = &accs[0][hl];
#pragma unroll
        for (int j = 0; j < 3; ++j) lacc[j * NR * TYQ] = 0.0;      // (read and written by this thread only: no barrier)
    }

    // One plane.  P,C,N hold planes t-1,t,t+1 of the own cells; D receives plane t+2; hc is the halo of plane t, hn
    // receives the halo of plane t+1; mc is the modulation of plane t, mn receives that of plane t+1.  The caller rotates
    // the roles instead of moving registers.
    auto step = [&](int t, float4(&P)[F], float4(&C)[F], float4(&N)[F], float4(&D)[F],
                    Halo<F, BC, COOP> &hc, Halo<F, BC, COOP> &hn, float4 &mc, float4 &mn) __attribute__((always_inline)) {
        const int bi = (t - t0) & 1;
        // per-cell sets: this plane's first LB level quads go out BEFORE the field loads below, so the wait for them at the
        // end of the plane (vmcnt retires in issue order) leaves the loads of the coming planes in flight
        load_lev(t);
#pragma unroll
        for (int i = 0; i < F; ++i) {
            if (!SX::has(i)) continue;
            const int k = SX::slot(i);
            lds[bi][k][ty + 1][q] = C[i];
            if constexpr (COOP) {
                if (hduty) reinterpret_cast<float *>(&lds[bi][k][hslot][0])[hcol] = hc.row[i];
            } else {
                if (hduty) lds[bi][k][hslot][q] = hc.row[i];
            }
        }
        // issue order = order of first use (vmcnt retires in issue order): the halo of t+1 is staged first at the next
        // plane, the own cells of t+2 are read there as t+1, the modulation of t+1 after that plane's functor
        load_halo(t + 1, hn);
        load_own(t + 2, D);
        load_mod(t + 1, mn);
        if constexpr (SX::count > 0) lds_barrier();

        Nbr n[F];
#pragma unroll
        for (int i = 0; i < F; ++i) {
            n[i].c = C[i];
            n[i].tm = P[i];
            n[i].tp = N[i];
            if (SX::has(i)) {
                n[i].xm = lds[bi][SX::slot(i)][ty][q];
                n[i].xp = lds[bi][SX::slot(i)][ty + 2][q];
            } else {
                n[i].xm = n[i].xp = f4(__builtin_nanf(""));      // never read by the functor (or the result says so)
            }
            float lft = lane_below(C[i].w);
            float rgt = lane_above(C[i].x);
            lft = ledge ? hc.ye[i] : lft;
            rgt = redge ? (BC ? hc.yr[i] : hc.ye[i]) : rgt;
            n[i].ym = make_float4(lft, C[i].x, C[i].y, C[i].z);
            n[i].yp = make_float4(C[i].y, C[i].z, C[i].w, rgt);
        }
        const float4 r = Fn::eval(n, prm);
        if constexpr (LACC) {
            double pl[3] = {0.0, 0.0, 0.0};
            stats_plane(r, keep, pl, smax, snan);
#pragma unroll
            for (int j = 0; j < 3; ++j) lacc[j * NR * TYQ] += pl[j];
        } else if constexpr (STATS) {
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

    Halo<F, BC, COOP> h0, h1;
    float4 w0[F], w1[F], w2[F], w3[F], m0, m1;
    load_own(t0 - 1, w0);
    load_own(t0, w1);
    load_own(t0 + 1, w2);
    load_halo(t0, h0);
    load_mod(t0, m0);
    for (int t = t0; t < t1; t += 4) {
        step(t, w0, w1, w2, w3, h0, h1, m0, m1);
        if (t + 1 >= t1) break;
        step(t + 1, w1, w2, w3, w0, h1, h0, m1, m0);
        if (t + 2 >= t1) break;
        step(t + 2, w2, w3, w0, w1, h0, h1, m0, m1);
        if (t + 3 >= t1) break;
        step(t + 3, w3, w0, w1, w2, h1, h0, m1, m0);
    }

    // combine: the waves of the workgroup through LDS, then one integer atomic per result for this sample.  Non-negative
    // floats order like their bit patterns and the NaN pattern lies above +inf: the unsigned maximum is the float maximum
    // with NaN sticky, across workgroups and across calls.
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) smax = fmaxf(smax, __shfl_xor(smax, o));
    const unsigned int ubits = __ballot(snan) ? 0x7fc00000u : __float_as_uint(smax);
    const int wv = hl >> 6;
    if constexpr (STATS) {
        // statistics: the maximum as below; the sums by shuffles, then LDS in wave order, then ONE slot of the workspace
        __shared__ double dred[3][NW];
        if constexpr (LACC) {
#pragma unroll
            for (int j = 0; j < 3; ++j) sacc[j] = lacc[j * NR * TYQ];
        }
        stats_wave(sacc);
        if ((hl & 63) == 0) {
            red[0][wv] = ubits;
#pragma unroll
            for (int j = 0; j < 3; ++j) dred[j][wv] = sacc[j];
        }
        __syncthreads();
        if (hl == 0) {
            unsigned int v = 0;
            double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                v = max(v, red[0][w]);
#pragma unroll
                for (int j = 0; j < 3; ++j) s[j] += dred[j][w];
            }
            if (v) atomicMax(g.score + b, v);
            stats_store(sets, slot, s[0], s[1], s[2]);
        }
        return;
    }
    if ((hl & 63) == 0) {
        red[0][wv] = ubits;
#pragma unroll
        for (int k = 0; k < NKMAX; ++k) red[1 + k][wv] = cnt[k];
    }
    __syncthreads();
    if (hl <= g.nk) {
        unsigned int v = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) v = hl == 0 ? max(v, red[0][w]) : v + red[hl][w];
        if (v) {
            if (hl == 0) atomicMax(g.score + b, v);
            else atomicAdd(g.count + (long long)(hl - 1) * g.cld + b, v);
        }
    }
}

// ------------------------------------------------------------------ host side
template <class Fn, int NR, int TYQ, class Sets, bool BC = false>
int launch_screen_tiled(SGeom &g, const typename Fn::Params &prm, hipStream_t st, const Sets &sets, const BCInfo *bc = nullptr)
{
    static_assert(2 * Staged<Fn>::FX * (NR + 2) * TYQ * 16 + (NKMAX + 1) * (NR * TYQ / 64) * 4 <= 160 * 1024, "tile does not fit the 160 KiB LDS");
    g.nXT = (g.X + NR - 1) / NR;
    g.nYT = (g.Y + 4 * TYQ - 1) / (4 * TYQ);
    for (int i = 0; i < Fn::F; ++i)            // a thread's place in a plane is a 32-bit byte offset (from one row before row 0)
        if (g.sX[i] < 0 || ((long long)(g.X + 2 + NR) * g.sX[i] + g.Y + 8) * 4 >= (1LL << 32)) return PRE_E_SHAPE;
    if (g.mod && (g.mX < 0 || ((long long)(g.X + NR) * g.mX + g.Y + 8) * 4 >= (1LL << 32))) return PRE_E_SHAPE;
    long long nb = g.B;                        // samples the grid covers: per-cell sets, whole groups of CELLS_G
    if constexpr (Sets::CELLS) {
        nb = (nb + CELLS_G - 1) / CELLS_G * CELLS_G;
        if (sets.qX < 0 || ((long long)(g.X + NR) * sets.qX + g.Y + 8) * 4 >= (1LL << 32)) return PRE_E_SHAPE;
    }
    long long tiles = nb * g.nXT * g.nYT;
    static const int per_cu = resident_per_cu(screen_march_kernel<Fn, NR, TYQ, Sets, BC>, NR * TYQ);
    int tSeg = pick_tseg(tiles, g.T, (long long)per_cu * chip_cus());
    if (TFREE_TSEG > 0 && g.tfree && tSeg > TFREE_TSEG) tSeg = TFREE_TSEG;     // (segments cost no window prologue then)
    g.tSeg = tSeg;
    g.nTSeg = (g.T + tSeg - 1) / tSeg;
    tiles *= g.nTSeg;
    if (tiles <= 0 || tiles * TYQ > 0xffffffffLL) return PRE_E_SHAPE;      // the dispatch packet counts work-items in 32 bits
    if constexpr (IsStats<Sets>::value)
        if (!stats_room(sets, tiles)) return PRE_E_NULL;                   // (never with the length the query entry gives)
    if constexpr (BC) {
        hipLaunchKernelGGL((screen_march_kernel<Fn, NR, TYQ, Sets, true>), dim3((unsigned)tiles), dim3(TYQ, NR), 0, st, g, prm, sets, *bc);
    } else {
        hipLaunchKernelGGL((screen_march_kernel<Fn, NR, TYQ, Sets, false>), dim3((unsigned)tiles), dim3(TYQ, NR), 0, st, g, prm, sets, NoBC{});
    }
    PRE_LAUNCH_CHECK();
    if constexpr (IsStats<Sets>::value) return stats_finish(sets, g.B, tiles / g.B, st);
    return PRE_OK;
}

// statistics: an upper bound of the workgroups per sample of any launch_screen on (T, X, Y), from the shape alone - the tiles
// below, and marches no shorter than min(T, 8) planes (pick_tseg stops above 8, TFREE_TSEG is 8)
inline long long stats_slots_ny(long long T, long long X, long long Y)
{
    static_assert(TFREE_TSEG == 0 || TFREE_TSEG >= 8, "marches of fewer than 8 planes: more workgroups than the bound");
    const int NR = Y >= 192 ? 8 : Y >= 96 ? 16 : 32, W = Y >= 192 ? 256 : Y >= 96 ? 128 : 64;
    return ((X + NR - 1) / NR) * ((Y + W - 1) / W) * ((T + 7) / 8);
}

template <class Fn, class Sets = ScalarSets, bool BC = false>
int launch_screen(SGeom &g, const typename Fn::Params &prm, hipStream_t st, const Sets &sets = Sets(), const BCInfo *bc = nullptr)
{
    // the tiles of star_march.h's launch()
    if (g.Y >= 192) return launch_screen_tiled<Fn, 8, 64, Sets, BC>(g, prm, st, sets, bc);
    if (g.Y >= 96) return launch_screen_tiled<Fn, 16, 32, Sets, BC>(g, prm, st, sets, bc);
    return launch_screen_tiled<Fn, 32, 16, Sets, BC>(g, prm, st, sets, bc);
}

template <template <int> class FnT, class P, class Sets = ScalarSets>
int launch_screen_mode(int mode, SGeom &g, const P &prm, hipStream_t st, const Sets &sets = Sets())
{
    if (mode == 0) return launch_screen<FnT<0>>(g, prm, st, sets);
    if (mode == 1) return launch_screen<FnT<1>>(g, prm, st, sets);
    return launch_screen<FnT<2>>(g, prm, st, sets);
}

// Null / empty / layout / range checks of everything an entry hands to the kernel, and the geometry.  No axis relabelling
// here: the sample's planes are [X,Y] with Y contiguous, or the library declines.
int prepare_screen(SGeom &g, const pre_field_t *const *fs, int nf, const pre_screen_t *s, int64_t B, int64_t T, int64_t X,
                   int64_t Y, int flags)
{
    const int rc = screen_args(fs, nf, s, NKMAX, B, T, X, Y, 8);
    if (rc) return rc;
    if (flags & ~(PRE_FLAG_HALO_X | PRE_FLAG_INTERIOR_T)) return PRE_E_UNSUPPORTED;
    for (int i = 0; i < nf; ++i)
        if (fs[i]->sY != 1) return PRE_E_UNSUPPORTED;              // (Nt-fastest views and the like: the caller falls back)
    if (Y % 4 != 0) return PRE_E_UNSUPPORTED;                      // (whole quads only)
    for (int i = 0; i < MAXF; ++i) {
        const bool on = i < nf;
        g.f[i] = on ? fs[i]->ptr : nullptr;
        g.sB[i] = on ? fs[i]->sB : 0; g.sT[i] = on ? fs[i]->sT : 0; g.sX[i] = on ? fs[i]->sX : 0;
    }
    g.mod = s->modulation; g.mT = s->mT; g.mX = s->mX;
    g.q = s->q; g.score = s->score; g.count = s->count; g.cld = s->count_ld;
    g.B = (int)B; g.T = (int)T; g.X = (int)X; g.Y = (int)Y;
    g.flags = flags;
    g.tfree = 0;
    g.ct = s->ct; g.cx = s->cx; g.cy = s->cy; g.nk = s->nk;
    return PRE_OK;
}

}  // namespace
