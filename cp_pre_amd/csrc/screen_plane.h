// screen_plane.h - the end of a plane (of a row, in the 1-D screen) that the three screens against calibrated sets share:
// screen_march.hip (libcp_pre_screen.so), screen_rows.hip (libcp_pre_screen1d.so) and screen_flat.hip
// (libcp_pre_screenflat.so).  The crop is a select, the score uses the guarded divide of the joint score pass, hw = q_k * m
// is one fp32 multiply with contraction off by pragma, the counts go compare -> wave mask -> population count -> scalar add.
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
