// screen_rows.h - the row march of the calibrated-set screen of the 1-D residuals, stated once for screen_rows.hip
// (libcp_pre_screen1d.so: |r| of one field set) and screen_rows_pair.hip (libcp_pre_screen1dpair.so: |r(a) - r(b)| of two
// field sets, the functor Paired<Fn> of paired_functor.h).  The number of field sets is Fn::F, 1 or 2: every register the
// march holds of a field (the four row roles, the edge scalar) is an array over the sets, the modulation, the end of a row,
// the combine step and the atomics do not depend on it.
//
// The march templates are star_march.h's (Star, Nbr, apply<>, Linear1, Burgers<MODE>, the lane shifts, the buffer
// descriptors' idiom, the XCD remap, star_from_dense27, shape_of, resident_per_cu, chip_cus).  screen_march_kernel treats
// [B,T,X] as [1,B,T,X] and marches over the batch: one workgroup would span many samples.  Here a sample is a PLANE of
// R rows x C columns, C the axis with unit stride (Nx-fastest: R = Nt, C = Nx; Nt-fastest: R = Nx, C = Nt), and a workgroup
// works on one sample only:
//   * a wave owns one column strip of 64 quads (256 columns) and marches a segment of rows: rows r-1, r, r+1 of its own
//     quads of every set in registers and row r+2 of every set in flight (march_kernel's four-role rotation: no register is
//     moved);
//   * the row neighbours (Nbr::xm / xp) are those registers, the column neighbours (ym / yp) come from the adjacent lane;
//     the wave's first and last lane fetch one edge scalar per set; tm / tp are zeros (apply<K_STAR7> does not multiply a
//     zero weight along that axis); rows and columns outside the sample are zero padding, what the residual passes compute;
//   * no LDS and no barrier inside the march: waves meet once, at the end.
// The end of a row is screen_march.hip's end of a plane (screen_plane.h): crop by select, guarded divide, hw = q_k * m without contraction, compare -> wave mask ->
// population count -> scalar add per level.  The waves of a workgroup are combined through LDS and the workgroup issues
// ONE integer atomicMax on the score's bits and nk integer atomicAdds for its sample: order-independent, so repeated
// calls and overlapping row slabs compose exactly and every run gives the same bytes.
//
// THE SPLIT (rows_split below; a pure function of B, R, C and the resident workgroups `slots`):
//   strips = ceil(C / 256)                          column strips of a sample
//   WS     = strips >= 3 ? 4 : strips               strips per workgroup (1, 2 or 4): a workgroup is 4 waves
//   NSEG   = 4 / WS                                 row segments per workgroup (4, 2 or 1)
//   nCT    = ceil(strips / WS)                      column tiles of 256 * WS columns (C > 1024: more than one)
//   rc     = R; while (B * nCT * ceil(R / rc) < slots && rc > 8 * NSEG) rc = ceil(rc / 2)
//                                                   rows per workgroup: halved until the chip is full or a segment would
//                                                   fall below 8 rows (a segment reads 2 rows for nothing)
//   nChunk = ceil(R / rc)                           workgroups along the rows of one sample
//   rSeg   = ceil(rc / NSEG)                        rows per wave segment
// Workgroup (b, chunk, ct), wave w: strip ct * WS + w % WS, rows [chunk * rc + (w / WS) * rSeg, + rSeg) cut to the chunk
// and to the counted rows [cr, R - cr).  A wave with no counted row or no column marches nothing.  slots >= 256 on every
// MI355X: for B * nCT * ceil(R / (8 * NSEG)) < 256 the split does not depend on it (tests/screen1d_helpers.py).
//
// The modulation m[R,C] is one more float4 stream through its own descriptor, shared by all samples: only lanes with a
// counted cell load it, and only for counted rows.  Block order: chunks and column tiles of a sample contiguous per XCD,
// the sample the slowest index (as screen_march_kernel: the XCDs walk different samples through the same rows).
//
// The buffer descriptors carry no record limit: every load of every set is guarded by the lane's `inb` and the row range.
//
// PER-CELL SETS (screen_rows_cells.hip, libcp_pre_screen1dcells.so): the kernel takes screen_plane.h's sets policy as the two
// 2-D marches do.  ScalarSets (the default) is everything above.  Under CellSets g.q is nk level FIELDS [R,C] shared by all
// samples (level stride sets.qK, row stride sets.qT, unit stride on C) and three things change, nothing else:
//   sets    a lane with a counted cell loads the quads of levels [0, LB) of row r (load_lev, as load_mod loads the modulation
//           quad: one wave-uniform descriptor per level and row, no record limit, guarded by `anykeep` and the counted row
//           range) as the FIRST loads of the row's step, ahead of the edge of r+1, the own quads of r+2 and the modulation
//           of r+1: vmcnt retires in issue order, so the wait for the level quads after the functor leaves those in flight.
//           LB = CellsBatch<Fn>: 16 unless the functor leaves no room; then later batches are fetched after the functor;
//   row     screen_plane_score + screen_plane_count<LB>: hw = ql[k][j] * m[j] in place of qk[k] * m[j];
//   order   the sample of a group of ROWS_CELLS_G is the fastest logical block index, then the column tile, the chunk, the
//           group: the workgroups an XCD runs together (xcd_remap makes them contiguous) are ROWS_CELLS_G samples at ONE
//           (chunk, tile) and read the same level quads from its L2.  nk = 10 level fields of a [200,512] plane are 4 MB, an
//           XCD's whole L2, against 0.4 MB of one sample's field: with the sample slowest every sample would drag 40 B of
//           levels per cell across the fabric against 4 B of field.  The grid covers whole groups; the surplus workgroups of
//           a partial last group return as a whole before the combine barrier.  rows_split does not know of it.
#pragma once
#include "screen_plane.h"

namespace {

constexpr int ROWS_NW = 4;                   // waves per workgroup
constexpr int ROWS_MINSEG = 8;               // fewest rows per wave segment the split goes down to
constexpr int ROWS_MAXSETS = 2;              // field sets a march reads: 1, or the truth and the prediction
// per-cell sets: the samples of a group, the fastest index of the block order (1: the order of the joint screens); a build
// constant of libcp_pre_screen1dcells.so, speed only
#ifndef PRE_SCREEN1DCELLS_GROUP
#define PRE_SCREEN1DCELLS_GROUP 16
#endif
constexpr int ROWS_CELLS_G = PRE_SCREEN1DCELLS_GROUP;
static_assert(ROWS_CELLS_G >= 1, "a group has at least one sample");

struct RGeom {
    const float *f[ROWS_MAXSETS];
    long long sB[ROWS_MAXSETS], sR[ROWS_MAXSETS];   // sample and row strides of each set (elements); columns have unit stride
    const float *mod;            // nullptr: m == 1
    long long mR;
    const float *q;              // device, nk levels (per-cell sets: nk level fields [R,C], strides in CellSets)
    unsigned int *score;         // [B]
    unsigned int *count;         // [nk][cld]
    long long cld;
    int B, R, C;
    int ws, nCT, rc, nChunk, rSeg;
    int cr, cc, nk;              // rows / columns per side left out of the counted region
};

struct RSplit { int ws, nCT, rc, nChunk, rSeg; };

RSplit rows_split(long long B, int R, int C, long long slots)
{
    RSplit s;
    const int strips = (C + 255) / 256;
    s.ws = strips >= 3 ? 4 : strips;
    const int nseg = ROWS_NW / s.ws;
    s.nCT = (strips + s.ws - 1) / s.ws;
    int rc = R;
    while (B * s.nCT * ((R + rc - 1) / rc) < slots && rc > ROWS_MINSEG * nseg) rc = (rc + 1) / 2;
    s.rc = rc;
    s.nChunk = (R + rc - 1) / rc;
    s.rSeg = (rc + nseg - 1) / nseg;
    return s;
}

// statistics: an upper bound of the workgroups per sample of rows_split on a plane of R rows x C columns, whatever `slots`:
// rc is halved only from above 8 * NSEG, so it stays >= min(R, 5)
inline long long stats_slots_rows(long long R, long long C)
{
    static_assert(ROWS_MINSEG >= 8, "shorter segments: more workgroups than the bound");
    const long long strips = (C + 255) / 256, ws = strips >= 3 ? 4 : strips;
    return ((strips + ws - 1) / ws) * ((R + 3) / 4);
}

// What the march evaluates per row: Fn::eval, except where the four unrolled row steps of the march would not round alike.
// Under fma contraction the compiler is free to fuse either product of a sum of two products, and for Burgers<3> (Nt-fastest,
// reference taps) it fused dx * D_t(u) + (dt * u) * D_x(u) as fma(dx, D_t, fl((dt u) D_x)) in the first step and as
// fma(dt u, D_x, fl(dx D_t)) in the other three: r of a row then depended, by 1-2 ulp, on the row's place in its wave's
// segment, and row slabs did not compose to the bits of the whole plane.  The specialisation states the order of the last
// three operations - the first form, which every step of Burgers<0> and Burgers<2> has - and leaves the stencil sums, which
// every step fused alike, to apply<>.  Registers, LDS and occupancy stay what they were.  Every other instantiation built
// rounds its four steps alike (read in the code objects).
template <class Fn>
struct RowsFn {
    static __device__ __forceinline__ float4 eval(const Nbr (&n)[Fn::F], const typename Fn::Params &p) { return Fn::eval(n, p); }
};
template <>
struct RowsFn<Burgers<3>> {
    static __device__ __forceinline__ float4 eval(const Nbr (&n)[1], const BurgersParams &p)
    {
#pragma clang fp contract(off)
        typedef float f32x2 __attribute__((ext_vector_type(2)));     // (a pair per operation: the packed fma of the other modes)
        const Nbr &u = n[0];
        const float4 dt = apply<K_Y3>(p.Dt, u), a = (p.dt * u.c) * apply<K_X3>(p.Dx, u), t = p.nu * apply<K_X3>(p.Dxx, u);
        const f32x2 dx = {p.dx, p.dx}, c3 = {p.c3, p.c3};
        // r = fma(-fl(nu D_xx), c3, fma(dx, D_t, fl(fl(dt u) D_x)))
        const f32x2 lo = __builtin_elementwise_fma(-f32x2{t.x, t.y}, c3, __builtin_elementwise_fma(dx, f32x2{dt.x, dt.y}, f32x2{a.x, a.y}));
        const f32x2 hi = __builtin_elementwise_fma(-f32x2{t.z, t.w}, c3, __builtin_elementwise_fma(dx, f32x2{dt.z, dt.w}, f32x2{a.z, a.w}));
        return make_float4(lo.x, lo.y, hi.x, hi.y);
    }
};

template <class Fn, class Sets = ScalarSets>
__global__ void __launch_bounds__(64 * ROWS_NW)
screen_rows_kernel(const RGeom g, const typename Fn::Params prm, const Sets sets)
{
    constexpr int NS = Fn::F;                      // field sets
    constexpr bool CELLS = Sets::CELLS;
    constexpr bool STATS = IsStats<Sets>::value;   // (per-sample statistics: no levels, no modulation, screen_plane.h)
    constexpr int LB = CellsBatch<Fn>::value;      // (per-cell sets: level quads held at once)
    static_assert(NS >= 1 && NS <= ROWS_MAXSETS, "one field per set, one or two sets");
    static_assert(64 * ROWS_NW >= NKMAX + 1, "one thread per result in the combine step");
    __shared__ unsigned int red[NKMAX + 1][ROWS_NW];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    [[maybe_unused]] const unsigned slot = L;      // (statistics: this workgroup's slot of the workspace)
    // per-cell sets: the sample of a group the fastest index; the last group is partial when B % ROWS_CELLS_G != 0
    const int bl = CELLS ? L % ROWS_CELLS_G : 0;
    if constexpr (CELLS) L /= ROWS_CELLS_G;
    const int ct = L % g.nCT; L /= g.nCT;
    const int ch = L % g.nChunk;
    const int b = CELLS ? (L / g.nChunk) * ROWS_CELLS_G + bl : L / g.nChunk;
    if constexpr (CELLS)
        if (b >= g.B) return;                      // (workgroup-uniform: no such sample in the last group; before the barrier)

    // this wave's strip and the rows it evaluates: its segment, cut to the chunk and to the counted rows
    const int strip = ct * g.ws + wv % g.ws;
    const int s0 = ch * g.rc + (wv / g.ws) * g.rSeg;
    const int r0 = max(s0, g.cr);
    const int r1 = min(min(s0 + g.rSeg, min(ch * g.rc + g.rc, g.R)), g.R - g.cr);
    const int y = strip * 256 + lane * 4;
    const bool inb = y < g.C;                      // (whole quads only: C % 4 == 0, checked by the host)
    const bool keep[4] = {inb && y >= g.cc && y < g.C - g.cc, inb && y + 1 >= g.cc && y + 1 < g.C - g.cc,
                          inb && y + 2 >= g.cc && y + 2 < g.C - g.cc, inb && y + 3 >= g.cc && y + 3 < g.C - g.cc};
    const bool anykeep = keep[0] || keep[1] || keep[2] || keep[3];

    [[maybe_unused]] float qk[NKMAX];              // (per-cell sets: a quad per level and row, load_lev)
    unsigned int cnt[NKMAX];
#pragma unroll
    for (int k = 0; k < NKMAX; ++k) {
        if constexpr (CELLS || STATS) qk[k] = 0.f;
        else qk[k] = k < g.nk ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g.q[k]))) : 0.f;
        cnt[k] = 0;
    }
    float smax = 0.f, sthr = 0.f;
    bool snan = false;
    [[maybe_unused]] double sacc[3] = {0.0, 0.0, 0.0};      // (statistics: sum r, sum |r|, sum r^2 of this lane's cells)

    if (r0 < r1 && strip * 256 < g.C) {            // (wave-uniform; no barrier in here)
        // column-halo duty: ONE edge scalar per lane and set (the column before the strip for the wave's first lane, the
        // column after it for its last lane); a partial strip's last quad takes its y+ cell from the next lane, which holds
        // zeros
        const bool ledge = lane == 0, redge = lane == 63;
        const bool eload = ledge ? (inb && y > 0) : (redge && inb && y + 4 < g.C);
        const int eoff4 = 4 * (ledge ? -1 : 4);
        // a row of this sample is a wave-uniform buffer descriptor, a lane's place in it a 32-bit byte offset (the host has
        // checked that 4 * C fits)
        const int voff = y * 4;
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        auto row = [&](int s, int r) __attribute__((always_inline)) {
            const float *p = g.f[s] + ((long long)b * g.sB[s] + (long long)r * g.sR[s]);
            return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, -1, 0x00020000);
        };
        auto load_own = [&](int r, float4 (&dst)[NS]) __attribute__((always_inline)) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (inb && r >= 0 && r < g.R) {
                    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(row(s, r), voff, 0, 0);
                    dst[s] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
                } else {
                    dst[s] = f4(0.f);
                }
            }
        };
        // (the edge scalar of row r is needed only when row r is evaluated: r < r1)
        auto load_edge = [&](int r, float (&e)[NS]) __attribute__((always_inline)) {
#pragma unroll
            for (int s = 0; s < NS; ++s)
                e[s] = (eload && r < r1) ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(row(s, r), voff + eoff4, 0, 0)) : 0.f;
        };
        auto load_mod = [&](int r, float4 &dst) __attribute__((always_inline)) {
            if constexpr (STATS) {
                dst = f4(1.0f);                    // (no modulation under this policy: no registers for it either)
            } else if (g.mod && anykeep && r < r1) {
                const float *p = g.mod + (long long)r * g.mR;
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(
                    __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, -1, 0x00020000), voff, 0, 0);
                dst = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
            } else {
                dst = f4(1.0f);
            }
        };

        // per-cell sets: the quads of levels [k0, k0 + LB) at row r, loaded like the modulation - only by lanes with a counted
        // cell and only for counted rows; a rim cell of a level field shares its quad with counted ones and is masked
        [[maybe_unused]] float4 ql[CELLS ? LB : 1];
        [[maybe_unused]] auto load_lev = [&](int r, int k0) __attribute__((always_inline)) {
            if constexpr (CELLS) {
#pragma unroll
                for (int k = 0; k < LB; ++k) {
                    if (anykeep && r < r1 && k0 + k < g.nk) {
                        const float *p = g.q + ((long long)(k0 + k) * sets.qK + (long long)r * sets.qT);
                        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(
                            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, -1, 0x00020000), voff, 0, 0);
                        ql[k] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
                    } else {
                        ql[k] = f4(0.f);
                    }
                }
            }
        };

        // One row.  P,C,N hold rows r-1,r,r+1 of the own quad of every set; D receives row r+2; ec / mc are the edge scalars
        // and the modulation of row r, en / mn receive those of row r+1.  The caller rotates the roles.
        auto step = [&](int r, float4 (&P)[NS], float4 (&C)[NS], float4 (&N)[NS], float4 (&D)[NS], float (&ec)[NS],
                        float (&en)[NS], float4 &mc, float4 &mn) __attribute__((always_inline)) {
            // per-cell sets: this row's first LB level quads go out BEFORE the field loads below (vmcnt retires in issue order)
            load_lev(r, 0);
            load_edge(r + 1, en);
            load_own(r + 2, D);
            load_mod(r + 1, mn);
            Nbr n[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                n[s].c = C[s];
                n[s].tm = n[s].tp = f4(0.f);
                n[s].xm = P[s];
                n[s].xp = N[s];
                float lft = lane_below(C[s].w);
                float rgt = lane_above(C[s].x);
                lft = ledge ? ec[s] : lft;
                rgt = redge ? ec[s] : rgt;
                n[s].ym = make_float4(lft, C[s].x, C[s].y, C[s].z);
                n[s].yp = make_float4(C[s].y, C[s].z, C[s].w, rgt);
            }
            const float4 res = RowsFn<Fn>::eval(n, prm);
            if constexpr (STATS) {
                stats_plane(res, keep, sacc, smax, snan);
            } else if constexpr (!CELLS) {
                screen_plane(res, mc, keep, g.nk, qk, cnt, smax, sthr, snan);
            } else {
                float ac[4], sv[4];
                screen_plane_score(res, mc, keep, ac, sv, smax, sthr, snan);
#pragma unroll
                for (int k0 = 0; k0 < NKMAX; k0 += LB) {
                    if (k0 >= g.nk) break;                     // (wave-uniform)
                    if (k0 > 0) load_lev(r, k0);
                    screen_plane_count<LB>(ac, sv, k0, g.nk, ql, cnt);
                }
            }
        };

        float4 w0[NS], w1[NS], w2[NS], w3[NS], m0, m1;
        float e0[NS], e1[NS];
        load_own(r0 - 1, w0);
        load_own(r0, w1);
        load_own(r0 + 1, w2);
        load_edge(r0, e0);
        load_mod(r0, m0);
        for (int r = r0; r < r1; r += 4) {
            step(r, w0, w1, w2, w3, e0, e1, m0, m1);
            if (r + 1 >= r1) break;
            step(r + 1, w1, w2, w3, w0, e1, e0, m1, m0);
            if (r + 2 >= r1) break;
            step(r + 2, w2, w3, w0, w1, e0, e1, m0, m1);
            if (r + 3 >= r1) break;
            step(r + 3, w3, w0, w1, w2, e1, e0, m1, m0);
        }
    }

    // combine: the waves of the workgroup through LDS, then one integer atomic per result for this sample.  Non-negative
    // floats order like their bit patterns and the NaN pattern lies above +inf: the unsigned maximum is the float maximum
    // with NaN sticky, across workgroups and across calls.
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) smax = fmaxf(smax, __shfl_xor(smax, o));
    const unsigned int ubits = __ballot(snan) ? 0x7fc00000u : __float_as_uint(smax);
    if constexpr (STATS) {
        // statistics: the maximum as below; the sums by shuffles, then LDS in wave order, then ONE slot of the workspace (a
        // wave that marched nothing holds zeros, so every workgroup stores its slot)
        __shared__ double dred[3][ROWS_NW];
        stats_wave(sacc);
        if (lane == 0) {
            red[0][wv] = ubits;
#pragma unroll
            for (int j = 0; j < 3; ++j) dred[j][wv] = sacc[j];
        }
        __syncthreads();
        if (tid == 0) {
            unsigned int v = 0;
            double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int w = 0; w < ROWS_NW; ++w) {
                v = max(v, red[0][w]);
#pragma unroll
                for (int j = 0; j < 3; ++j) s[j] += dred[j][w];
            }
            if (v) atomicMax(g.score + b, v);
            stats_store(sets, slot, s[0], s[1], s[2]);
        }
        return;
    }
    if (lane == 0) {
        red[0][wv] = ubits;
#pragma unroll
        for (int k = 0; k < NKMAX; ++k) red[1 + k][wv] = cnt[k];
    }
    __syncthreads();
    if (tid <= g.nk) {
        unsigned int v = 0;
#pragma unroll
        for (int w = 0; w < ROWS_NW; ++w) v = tid == 0 ? max(v, red[0][w]) : v + red[tid][w];
        if (v) {
            if (tid == 0) atomicMax(g.score + b, v);
            else atomicAdd(g.count + (long long)(tid - 1) * g.cld + b, v);
        }
    }
}

// ------------------------------------------------------------------ host side
template <class Fn, class Sets = ScalarSets>
int launch_rows(RGeom &g, const typename Fn::Params &prm, hipStream_t st, const Sets &sets = Sets())
{
    static const int per_cu = resident_per_cu(screen_rows_kernel<Fn, Sets>, 64 * ROWS_NW);
    const RSplit s = rows_split(g.B, g.R, g.C, (long long)per_cu * chip_cus());
    g.ws = s.ws; g.nCT = s.nCT; g.rc = s.rc; g.nChunk = s.nChunk; g.rSeg = s.rSeg;
    long long nb = g.B;                        // samples the grid covers: per-cell sets, whole groups of ROWS_CELLS_G
    if constexpr (Sets::CELLS) nb = (nb + ROWS_CELLS_G - 1) / ROWS_CELLS_G * ROWS_CELLS_G;
    const long long wgs = nb * g.nChunk * g.nCT;
    if (wgs <= 0 || wgs * 64 * ROWS_NW > 0xffffffffLL) return PRE_E_SHAPE;      // the dispatch packet counts work-items in 32 bits
    if constexpr (IsStats<Sets>::value)
        if (!stats_room(sets, wgs)) return PRE_E_NULL;                          // (never with the length the query entry gives)
    hipLaunchKernelGGL((screen_rows_kernel<Fn, Sets>), dim3((unsigned)wgs), dim3(64 * ROWS_NW), 0, st, g, prm, sets);
    PRE_LAUNCH_CHECK();
    if constexpr (IsStats<Sets>::value) return stats_finish(sets, g.B, wgs / g.B, st);
    return PRE_OK;
}

// Null / empty / range / shape / layout checks of everything an entry hands to the kernel, and the geometry, for `ns` field
// sets u[i] with strides[i] (B, Nt, Nx).  *nt_fast: the unit-stride axis is Nt (rows = Nx); the caller relabels its star
// weights with it.  Every set and the modulation must have their unit stride on the SAME axis.
int prepare_rows(RGeom &g, int *nt_fast, const float *const *u, const int64_t *const *strides, int ns, const pre_screen_t *s,
                 int64_t B, int64_t T, int64_t X, int flags)
{
    if (ns < 1 || ns > ROWS_MAXSETS) return PRE_E_RANGE;
    for (int i = 0; i < ns; ++i)
        if (!u[i] || !strides[i]) return PRE_E_NULL;
    if (!s || !s->q || !s->score || !s->count || B <= 0 || T <= 0 || X <= 0) return PRE_E_NULL;
    if (s->nk < 1 || s->nk > PRE_SCREEN_MAX_LEVELS || s->ct < 0 || s->cx < 0 || s->cy != 0) return PRE_E_RANGE;
    if (s->count_ld < B) return PRE_E_NULL;
    if (B > 0x7fffffff || T > 0x7fffffff || X > 0x7fffffff) return PRE_E_SHAPE;
    if ((double)T * (double)X >= 4294967296.0) return PRE_E_SHAPE;                        // the counts are 32-bit
    if (flags) return PRE_E_UNSUPPORTED;
    const bool mod = s->modulation != nullptr;
    bool nx = !mod || s->mX == 1, nt = !mod || s->mT == 1;
    for (int i = 0; i < ns; ++i) {
        nx = nx && strides[i][2] == 1;
        nt = nt && strides[i][1] == 1;
    }
    if (nx) *nt_fast = 0;
    else if (nt) *nt_fast = 1;
    else return PRE_E_UNSUPPORTED;               // no unit-stride axis, or not the one of the modulation and of every set
    const int64_t R = *nt_fast ? X : T, C = *nt_fast ? T : X;
    if (C % 4 != 0) return PRE_E_UNSUPPORTED;    // (whole quads only)
    if (C > (1 << 28)) return PRE_E_SHAPE;       // a lane's place in a row is a 32-bit byte offset
    for (int i = 0; i < ROWS_MAXSETS; ++i) {     // (a set the march does not read repeats the first: never a stray pointer)
        const int k = i < ns ? i : 0;
        g.f[i] = u[k]; g.sB[i] = strides[k][0]; g.sR[i] = *nt_fast ? strides[k][2] : strides[k][1];
    }
    g.mod = s->modulation; g.mR = *nt_fast ? s->mX : s->mT;
    g.q = s->q; g.score = s->score; g.count = s->count; g.cld = s->count_ld;
    g.B = (int)B; g.R = (int)R; g.C = (int)C;
    g.cr = *nt_fast ? s->cx : s->ct; g.cc = *nt_fast ? s->ct : s->cx; g.nk = s->nk;
    return PRE_OK;
}

// the star of a 3x3 kernel K[a][c] (a over Nt, c over Nx) on the plane's axes: rows -> x, columns -> y; false if a corner
// holds weight
bool rows_star_from_dense9(const float *K, int nt_fast, Star *s)
{
    if (K[0] != 0.f || K[2] != 0.f || K[6] != 0.f || K[8] != 0.f) return false;
    const float tm = K[1], tp = K[7], xm = K[3], xp = K[5];
    *s = nt_fast ? Star{K[4], 0.f, 0.f, xm, xp, tm, tp} : Star{K[4], 0.f, 0.f, tm, tp, xm, xp};
    return true;
}

// a checked tap list (2 offsets per tap: Nt, Nx) as a dense 3x3 kernel; PRE_E_SHAPE for an offset beyond +-3, *star false
// for a tap off the 5-point star
int rows_dense9_of_taps(const float *tap_w, const int32_t *tap_off, int ntaps, float (&k9)[9], bool *star)
{
    for (int i = 0; i < 9; ++i) k9[i] = 0.f;
    *star = true;
    for (int i = 0; i < ntaps; ++i) {
        const int dt = tap_off[2 * i], dx = tap_off[2 * i + 1];
        if (dt < -3 || dt > 3 || dx < -3 || dx > 3) return PRE_E_SHAPE;
        if ((dt != 0 && dx != 0) || dt < -1 || dt > 1 || dx < -1 || dx > 1) { *star = false; continue; }
        k9[(dt + 1) * 3 + (dx + 1)] += tap_w[i];
    }
    return PRE_OK;
}

// The Burgers functor's parameters and tap structure on the plane's axes.  Burgers<0>: D_t purely along the rows, D_x / D_xx
// purely along the columns (Nx-fastest); Burgers<3>: the other way round (Nt-fastest); anything else is the general star,
// mode 2 (as pre_residual_burgers_f32 picks its mode).  PRE_E_UNSUPPORTED for weight on a corner.
int rows_burgers_params(BurgersParams &prm, int *mode, int nt_fast, const float *K_t, const float *K_x, const float *K_xx, float dx,
                        float dt, float nu, float c3)
{
    if (!rows_star_from_dense9(K_t, nt_fast, &prm.Dt) || !rows_star_from_dense9(K_x, nt_fast, &prm.Dx) ||
        !rows_star_from_dense9(K_xx, nt_fast, &prm.Dxx))
        return PRE_E_UNSUPPORTED;
    prm.dx = dx; prm.dt = dt; prm.nu = nu; prm.c3 = c3;
    const Shape a = shape_of(prm.Dt), b2 = shape_of(prm.Dx), c2 = shape_of(prm.Dxx);
    *mode = (!nt_fast && !a.y && !b2.x && !c2.x) ? 0 : (nt_fast && !a.x && !b2.y && !c2.y) ? 3 : 2;
    return PRE_OK;
}

}  // namespace
