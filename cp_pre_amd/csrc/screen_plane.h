// screen_plane.h - the end of a plane (of a row, in the 1-D screen) that the three screens against calibrated sets share:
// screen_march.hip (libcp_pre_screen.so), screen_rows.hip (libcp_pre_screen1d.so) and screen_flat.hip
// (libcp_pre_screenflat.so).  The crop is a select, the score uses the guarded divide of the joint score pass, hw = q_k * m
// is one fp32 multiply with contraction off by pragma, the counts go compare -> wave mask -> population count -> scalar add.
// Further down: the same end of a plane for per-cell level fields (CellSets), and the one of the per-sample statistics
// (StatSets: fp64 sums and max |r| in place of score and counts; screen_stats.hip, screen_rows_stats.hip).
#pragma once
#include "star_march.h"
#include "guarded_divide.h"
#include "../../include/cp_pre_screen.h"

namespace {

static_assert(PRE_SCREEN_MAX_LEVELS == 16, "the level loop of screen_plane is unrolled 16 times");
constexpr int NKMAX = PRE_SCREEN_MAX_LEVELS;

// The guarded divide of calib.hip's js_update (a translation unit of libcp_pre_hip.so), stated once in guarded_divide.h:
// the running maximum m of av / sv, bitwise what dividing every element gives.  Only a candidate that can raise the
// maximum pays for the IEEE division: a cell is skipped only if p = thr * sv is a normal number and av <= p, which that
// header shows to imply fl(av / sv) <= m for every fp32 input.  A NaN av or sv fails the compare and reaches the divide,
// 0/0 reaches it because p is then no normal number; a NaN quotient sets the sticky flag.
__device__ __forceinline__ void score_update(float av, float sv, float &m, float &thr, bool &nan)
{
    guarded_max_update(av, sv, m, thr, nan);
}

// The end of one plane.  r: the residual quad, mm: its modulation, keep[j]: cell j is counted.  qk / cnt: the levels and
// their wave-wide counts, both wave-uniform (scalar registers: no vector register per level).
// No fma contraction in here: hw = q * m rounds as coverage_levels.o's product does (csrc/Makefile), whatever the flags of
// the including file, which must stay those of star_march.o so that the functors round as the residual passes do.
__device__ __forceinline__ void screen_plane(const float4 &r, const float4 &mm, const bool (&keep)[4], int nk,
                                             const float (&qk)[NKMAX], unsigned int (&cnt)[NKMAX], float &m, float &thr, bool &nan)
{
#pragma clang fp contract(off)
    const float rv[4] = {r.x, r.y, r.z, r.w}, mv[4] = {mm.x, mm.y, mm.z, mm.w};
    float ac[4], sv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = fabsf(rv[j]);
        // a cell outside the counted region: |r| = 0 over m = 1 for the score (never a candidate), NaN for the counts
        // (outside at every level) - selects, so that whatever it holds stays where it is
        sv[j] = keep[j] ? mv[j] : 1.0f;
        score_update(keep[j] ? a : 0.0f, sv[j], m, thr, nan);
        ac[j] = keep[j] ? a : __builtin_nanf("");
    }
#pragma unroll
    for (int k = 0; k < NKMAX; ++k) {
        if (k < nk) {                                        // (wave-uniform)
            unsigned int c = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float hw = qk[k] * sv[j];
                c += (unsigned int)__popcll(__builtin_amdgcn_fcmpf(ac[j], hw, 5));      // 5: ordered <= (NaN: outside)
            }
            cnt[k] += c;
        }
    }
}

// What the per-cell screen (screen_cells.hip) adds to the two marches, as compile-time constants of its library.
// CELLS_G: the samples of a group, the fastest index of its block order (1: the order of the joint screens).
#ifndef PRE_SCREENCELLS_GROUP
#define PRE_SCREENCELLS_GROUP 16
#endif
constexpr int CELLS_G = PRE_SCREENCELLS_GROUP;
static_assert(CELLS_G >= 1, "a group has at least one sample");
// The sets a launch screens against, a compile-time policy of the two marches and their last kernel argument.  ScalarSets
// (the default): g.q is nk wave-uniform levels.  CellSets: g.q is nk level FIELDS [T,X,Y] shared by all samples, with unit
// stride on the fields' unit-stride axis; a thread loads nk level quads per plane next to the modulation quad.
struct ScalarSets { static constexpr bool CELLS = false; };
struct CellSets {
    static constexpr bool CELLS = true;
    long long qK, qT, qX;      // level, marched-plane and row strides of g.q in elements (the merged-row march has no rows)
};
// CellsBatch<Fn>: the level quads a thread holds ACROSS the functor.  NKMAX: all of a plane's quads are issued before its
// field loads and counted after its functor; a functor whose instantiation would carry scratch with 16 more quads gets fewer
// (screen_cells.hip, screen_cells_pair.hip), and the quads beyond that first batch are fetched after the functor, a batch at a
// time.
// CellsLate<Fn>: the size of those later batches.  After the functor its neighbourhood is dead, so a functor that has room
// for ONE quad across its evaluation (the paired NS momentum: CellsBatch 1) can still take the other fifteen in one batch
// and one wait; by default the later batches have the first one's size.  Whole batches: (NKMAX - CellsBatch) % CellsLate == 0.
#ifndef PRE_SCREENCELLS_BATCH
#define PRE_SCREENCELLS_BATCH 16
#endif
static_assert(PRE_SCREENCELLS_BATCH >= 1 && PRE_SCREENCELLS_BATCH <= NKMAX && NKMAX % PRE_SCREENCELLS_BATCH == 0, "whole batches");
template <class Fn, class = void> struct CellsBatch { static constexpr int value = PRE_SCREENCELLS_BATCH; };
template <class Fn, class = void> struct CellsLate { static constexpr int value = CellsBatch<Fn>::value; };

// The same end of a plane for per-cell levels (screen_cells.hip): ql[k] is the quad of level k's field at the thread's four
// cells, so hw = ql[k][j] * m[j], the product of pre_cov_levels_f32 with a level field (q_ld != 0); without a modulation
// mm is 1 and 1.0f * q == q exactly, NaN, inf and sign included.  In two parts, so that a functor that leaves no room for
// nk quads can take them in batches: the score and the masked |r| once per plane, then the counts of levels [k0, k0 + NB).
__device__ __forceinline__ void screen_plane_score(const float4 &r, const float4 &mm, const bool (&keep)[4], float (&ac)[4],
                                                   float (&sv)[4], float &m, float &thr, bool &nan)
{
    const float rv[4] = {r.x, r.y, r.z, r.w}, mv[4] = {mm.x, mm.y, mm.z, mm.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = fabsf(rv[j]);
        sv[j] = keep[j] ? mv[j] : 1.0f;
        score_update(keep[j] ? a : 0.0f, sv[j], m, thr, nan);
        ac[j] = keep[j] ? a : __builtin_nanf("");
    }
}

template <int NB>
__device__ __forceinline__ void screen_plane_count(const float (&ac)[4], const float (&sv)[4], int k0, int nk,
                                                   const float4 (&ql)[NB], unsigned int (&cnt)[NKMAX])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        if (k0 + k < nk) {                                   // (wave-uniform)
            const float qv[4] = {ql[k].x, ql[k].y, ql[k].z, ql[k].w};
            unsigned int c = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float hw = qv[j] * sv[j];
                c += (unsigned int)__popcll(__builtin_amdgcn_fcmpf(ac[j], hw, 5));      // 5: ordered <= (NaN: outside)
            }
            cnt[k0 + k] += c;
        }
    }
}

// ---- per-sample statistics of the residual (screen_stats.hip, screen_rows_stats.hip: libcp_pre_screenstats.so) ------------
// StatSets, the third set policy of the three marches: no levels and no modulation.  A sample is reduced to sum r, sum |r|,
// sum r^2 and max |r| over its counted cells.  The maximum goes where the score goes (integer atomicMax on the bit pattern).
// The sums are fp64 from the first addition and see no atomic: a thread adds into three accumulators, a wave combines them by
// shuffles, a workgroup by LDS in wave order, and the workgroup STORES its three partials into its own slot of a caller's
// workspace, ws[slot][3] with slot the workgroup's logical index (the sample is its slowest part, so a sample's slots are
// contiguous).  A second launch on the same stream (stats_finish) adds each sample's slots in index order into sums: the
// same inputs and the same sequence of calls give the same bytes.  A workgroup with nothing to count stores zeros.
struct StatSets {
    static constexpr bool CELLS = false;
    double *ws;                // device, [workgroups of the launch][3]
    long long ws_len;          // doubles the caller provided
    double *sums;              // device, [3][sum_ld]: sum r, sum |r|, sum r^2, add-accumulated across calls
    long long sum_ld;
};
template <class Sets> struct IsStats { static constexpr bool value = false; };
template <> struct IsStats<StatSets> { static constexpr bool value = true; };

// Where a thread's three fp64 accumulators live between planes in screen_march_kernel: in registers, or (true) in a slot of
// its own in LDS, read, added to and written back once per plane.  The NS momentum functor in the reference's tap structure
// takes 129-131 registers with them where the level screen takes 125: one step past the 128 at which TWO of its 512-thread
// workgroups fit a CU (holding the kernel to four waves by its launch bounds gives 12 bytes of scratch instead).  With the
// accumulators in LDS - 12 KiB more per workgroup, still two per CU - it takes 125 (csrc/resources.sh; measured in DESIGN
// 4.30).  The y-fixed structure stays above 128 either way (133 in registers, 129 in LDS; the level screen 127) and keeps
// its registers.
template <class Fn> struct StatsLdsAcc { static constexpr bool value = false; };
template <> struct StatsLdsAcc<NSMomentum<0>> { static constexpr bool value = true; };

// The end of a plane under StatSets.  A cell outside the counted region contributes exactly nothing (selects: 0 to the
// maximum, +0.0 to the sums, whatever it holds).  Inside it the fp32 r is widened and every addition is fp64: (double) r,
// its absolute value and its square, which is exact in fp64.  The maximum stays fp32 with a sticky NaN, the score's max with
// m == 1 and no divide: bitwise what score_update(a, 1.0f, ...) keeps.
__device__ __forceinline__ void stats_plane(const float4 &r, const bool (&keep)[4], double (&acc)[3], float &m, bool &nan)
{
    const float rv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = keep[j] ? fabsf(rv[j]) : 0.0f;
        if (a != a) nan = true;
        else if (a > m) m = a;
        const double d = keep[j] ? (double)rv[j] : 0.0;
        acc[0] += d;
        acc[1] += fabs(d);
        acc[2] += d * d;
    }
}

// the three accumulators of a wave in every lane: a butterfly, the same order on every run
__device__ __forceinline__ void stats_wave(double (&acc)[3])
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[j] += __shfl_xor(acc[j], o);
    }
}

// one thread of a workgroup: its slot of the workspace (plain stores)
__device__ __forceinline__ void stats_store(const StatSets &sets, unsigned slot, double s0, double s1, double s2)
{
    double *p = sets.ws + 3ull * slot;
    p[0] = s0; p[1] = s1; p[2] = s2;
}

// the second launch: thread (j, b) adds the S slots of sample b in index order into sums[j][b]
template <class Sets>
__global__ void __launch_bounds__(256) stats_finish_kernel(const Sets sets, int B, int S)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3ll * B) return;
    const int j = (int)(i / B), b = (int)(i % B);
    const double *p = sets.ws + 3ll * b * S + j;
    double s = 0.0;
    for (int k = 0; k < S; ++k) s += p[3ll * k];
    sets.sums[(long long)j * sets.sum_ld + b] += s;
}

// host: does the workspace hold a launch of `wgs` workgroups?  (asked before the launch)
inline bool stats_room(const StatSets &sets, long long wgs) { return 3 * wgs <= sets.ws_len; }

// host: the second launch, after a march of S workgroups per sample (a template, as its kernel: only a unit that launches
// a march under StatSets holds either)
template <class Sets>
int stats_finish(const Sets &sets, int B, long long S, hipStream_t st)
{
    hipLaunchKernelGGL((stats_finish_kernel<Sets>), dim3((unsigned)((3ll * B + 255) / 256)), dim3(256), 0, st, sets, B, (int)S);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}

// screen_plane with a level quad per k in place of the wave-uniform qk[]
__device__ __forceinline__ void screen_plane_cells(const float4 &r, const float4 &mm, const bool (&keep)[4], int nk,
                                                   const float4 (&ql)[NKMAX], unsigned int (&cnt)[NKMAX], float &m, float &thr,
                                                   bool &nan)
{
    float ac[4], sv[4];
    screen_plane_score(r, mm, keep, ac, sv, m, thr, nan);
    screen_plane_count<NKMAX>(ac, sv, 0, nk, ql, cnt);
}

}  // namespace
