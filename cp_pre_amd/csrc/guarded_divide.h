// guarded_divide.h - the running maximum of av / sv that the joint score pass (calib.hip: js_update) and the screens against
// calibrated sets (screen_plane.h: score_update) keep per lane, stated once.  Host and device: tests/c_abi/
// guarded_divide_main.cpp runs this very function on the CPU against straight division.
//
// max_i fl(av_i / sv_i) with an IEEE division on every element would make the passes VALU-bound (a correctly rounded fp32
// divide is ~10 instructions).  A lane keeps its exact running maximum m and thr = fl(m (1 - 2^-20)), and a cell first
// forms p = fl(thr * sv): it is SKIPPED only if p is a normal number and av <= p; everything else pays for the divide.
//
// Why a skipped cell cannot raise the maximum, for every fp32 input (u = 2^-24, av >= 0 as both callers pass |r|):
//  - p normal and av <= p: p is finite and positive, so thr > 0, sv > 0, av is finite, and m >= thr > 0 is finite (an
//    infinite m has thr = inf and p = inf or NaN).  p >= 2^-126 is the result of one correctly rounded multiply, whose
//    error is at most half an ulp of the RESULT: p (1 - u) <= thr sv, so the exact quotient av / sv <= thr / (1 - u).
//  - m >= 2^-126: thr = fl(m (1 - 2^-20)) <= m (1 - 2^-20) + max(u thr, 2^-150) <= m (1 - 2^-20 + 2^-24), whether thr came
//    out normal (relative error u) or subnormal (absolute error 2^-150 <= 2^-24 m).  Then av / sv <= m (1 - 2^-20 + 2^-24)
//    / (1 - 2^-24) < m.
//  - m < 2^-126 (subnormal): thr <= m by monotone rounding, so av / sv <= m / (1 - u) < m + 2^-150, less than half a
//    subnormal step above m.
//  - in both cases fl(av / sv) <= m, because rounding is monotone and m is an fp32 number.  A NaN av, sv or thr makes
//    `av <= p` false.
//  - a SUBNORMAL p breaks the first step: its error is absolute, up to 2^-150, and relative to p unbounded.  m = 3 * 2^-149,
//    sv = 0.5, av = 2 * 2^-149: thr rounds back to m, p to 2 * 2^-149, yet av / sv = 4 * 2^-149 > m.  The same with m and sv
//    normal: m = 0x1.a30fecp-107, sv = 0x1.d710bep-30, av = 0x1.819p-136 has av <= p, yet av / sv = 0x1.a3112cp-107 > m.
//    An INFINITE p hides inf / inf: m > 0, sv = inf, av = inf has av <= p, yet av / sv is NaN.  (Testing sv for "normal"
//    instead of p, as this code did before, covers none of the three.)
//  - sv == 0 (0/0 is NaN, x/0 inf: p is 0 or NaN), sv < 0 (p <= 0) and m == 0 (thr == 0, p == 0 or NaN) all divide.
// A NaN quotient sets the sticky flag; a quotient <= 0 (negative modulation) never raises the maximum.
#pragma once

#if defined(__HIPCC__)
#define PRE_GD_FN __host__ __device__ __forceinline__
#else
#define PRE_GD_FN inline
#endif

PRE_GD_FN void guarded_max_update(float av, float sv, float &m, float &thr, bool &nan)
{
    // No fma contraction in here, whatever the flags of the including file (screen_plane.h's includers keep star_march.o's).
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    // (p normal: two plain compares against the smallest and the largest normal number - a NaN p has failed `av <= p`
    // already.  The class test - isnormal - cost the screen kernels one to nine vector registers, one of them its last
    // free ones: csrc/resources.sh.)
    const float p = thr * sv;
    if (!(av <= p) || p < 1.17549435e-38f || p > 3.40282347e+38f) {
        const float q = av / sv;
        if (q != q) nan = true;
        else if (q > m) { m = q; thr = m * 0.99999905f; }          // 1 - 2^-20, exact in fp32
    }
}

#undef PRE_GD_FN
