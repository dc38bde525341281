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

}  // namespace
