// guarded_divide_main.cpp - guarded_max_update of cp_pre_amd/csrc/guarded_divide.h on the CPU: the running maximum of
// av / sv that the joint score pass and the screens keep per lane, against straight division.  A cell may be skipped only
// if fl(av / sv) <= m, so after every cell the guarded maximum must equal the plain one, bit for bit, and the NaN flags
// must agree.  tests/test_calib_ref_cpu.py builds this file with the host compiler (no fma contraction) and runs it.
//
// Regimes (a triple is a state m reached through the function itself, then one candidate av over sv):
//   grid     m, av = {1, 1.5, 1.75, 1 + 2^-23, 2 - 2^-23} x 2^e with e from -149 to -90, sv = 2^-40 .. 2^19 (subnormal m,
//            subnormal thr * sv with everything else normal, and the normal cells next to them); then sv = 2^-149 .. 2^-90
//            under an m that puts thr * sv at the subnormal edge; the candidate presented after the cell that sets m
//            and, in a second run, before it
//   edge     for every (m, sv) of a coarser grid: av at fl(thr * sv) and 1, 2 ulp below and above it
//   random   seeded triples with m, sv, av / sv in the normal range, av / sv within a few 2^-20 of m
//   special  0, -0, inf, NaN, negative and subnormal sv, inf and NaN av, against every state of m
// Per regime the program prints how many candidates were skipped and how many divided; a regime with either count zero
// fails (a sweep that never skips proves nothing), as does any mismatch.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <initializer_list>

#include "../../cp_pre_amd/csrc/guarded_divide.h"

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float from_bits(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

struct Plain { float m = 0.f; bool nan = false; };
static void plain_update(float av, float sv, Plain &p)
{
    volatile float q = av / sv;                  // (volatile: one rounding to fp32, whatever the host's evaluation method)
    if (q != q) p.nan = true;
    else if (q > p.m) p.m = q;
}

struct Regime { const char *name; long long skipped = 0, divided = 0, bad = 0; };

// one candidate against a state: counts the route it took and compares with the plain maximum
static void candidate(Regime &r, float av, float sv, float &m, float &thr, bool &nan, Plain &p)
{
    const float pr = thr * sv;
    const bool skip = (av <= pr) && isnormal(pr);                // (restated only to COUNT the route; the result is compared)
    (skip ? r.skipped : r.divided)++;
    guarded_max_update(av, sv, m, thr, nan);
    plain_update(av, sv, p);
    if (bits(m) != bits(p.m) || nan != p.nan) {
        if (r.bad++ < 8)
            printf("%s: MISMATCH av=%a sv=%a guarded m=%a nan=%d plain m=%a nan=%d\n", r.name, av, sv, m, (int)nan, p.m, (int)p.nan);
    }
}

// the state "maximum m0" reached through the function: one cell m0 / 1
static void reach(float m0, float &m, float &thr, bool &nan, Plain &p)
{
    m = 0.f; thr = 0.f; nan = false; p = Plain();
    guarded_max_update(m0, 1.0f, m, thr, nan);
    plain_update(m0, 1.0f, p);
}

static const float MANT[5] = {1.0f, 1.5f, 1.75f, 1.00000011920928955078125f, 1.99999988079071044921875f};

int main()
{
    Regime grid{"grid"}, edge{"edge"}, rnd{"random"}, special{"special"};
    float m, thr;
    bool nan;
    Plain p;

    // ---- grid: every exponent triple across the subnormal / normal boundary of m, of thr * sv and of av
    for (int em = -149; em <= -90; ++em)
        for (int es = -40; es <= 19; ++es)                       // sv = 2^es: thr * sv spans 2^-189 .. 2^-71
            for (int ea = -149; ea <= -90; ++ea) {
                const int im = (em + es + ea) & 3, is = (em + 2 * es + ea) % 5, ia = (em + es + 3 * ea) % 5;
                const float m0 = ldexpf(MANT[im], em), sv = ldexpf(MANT[is < 0 ? -is : is], es), av = ldexpf(MANT[ia < 0 ? -ia : ia], ea);
                if (m0 == 0.f || av == 0.f) continue;
                reach(m0, m, thr, nan, p);
                candidate(grid, av, sv, m, thr, nan, p);         // after the cell that sets m
                m = 0.f; thr = 0.f; nan = false; p = Plain();    // before it: the candidate first, then the cell that would set m
                candidate(grid, av, sv, m, thr, nan, p);
                candidate(grid, m0, 1.0f, m, thr, nan, p);
            }
    // the same edge reached from the other side: sv = 2^-149 .. 2^-90 (subnormal and small normal modulations) under an m
    // that puts thr * sv within 2^-24 .. 2^6 of the smallest normal number, av within 2^-3 .. 2^3 of the product
    for (int es = -149; es <= -90; ++es)
        for (int d = -24; d <= 6; ++d)
            for (int da = -3; da <= 3; ++da)
                for (int k = 0; k < 5; ++k) {
                    const int em = -126 - es + d;
                    if (em > 127) continue;
                    const float m0 = ldexpf(MANT[k], em), sv = ldexpf(MANT[(k + d + 24) % 5], es);
                    const float av = ldexpf(MANT[(k + da + 3) % 5], em + es + da);
                    if (sv == 0.f || av == 0.f || !(m0 < INFINITY)) continue;
                    reach(m0, m, thr, nan, p);
                    candidate(grid, av, sv, m, thr, nan, p);
                    m = 0.f; thr = 0.f; nan = false; p = Plain();
                    candidate(grid, av, sv, m, thr, nan, p);
                    candidate(grid, m0, 1.0f, m, thr, nan, p);
                }
    // the two counterexamples of the unguarded form, stated as found
    {
        reach(from_bits(3u), m, thr, nan, p);
        candidate(grid, from_bits(2u), 0.5f, m, thr, nan, p);
        reach(0x1.a30fecp-107f, m, thr, nan, p);
        candidate(grid, 0x1.819p-136f, 0x1.d710bep-30f, m, thr, nan, p);
    }

    // ---- edge: av at fl(thr * sv) and up to 2 ulp either side
    for (int em = -149; em <= 100; em += 1)
        for (int es = -60; es <= 60; es += 3)
            for (int k = 0; k < 5; ++k) {
                const float m0 = ldexpf(MANT[k], em), sv = ldexpf(MANT[(k + es + 60) % 5], es);
                if (m0 == 0.f || !(m0 < INFINITY)) continue;
                for (int d = -2; d <= 2; ++d) {
                    reach(m0, m, thr, nan, p);
                    const float t = m0 * 0.99999905f;
                    volatile float pr = t * sv;
                    if (!(pr > 0.f) || !(pr < INFINITY)) continue;
                    const int64_t b = (int64_t)bits(pr) + d;
                    if (b <= 0 || b >= 0x7f800000) continue;
                    candidate(edge, from_bits((uint32_t)b), sv, m, thr, nan, p);
                }
            }

    // ---- random: the normal range, quotients close to m (xorshift64*, fixed seed)
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; };
    for (long long i = 0; i < 4000000; ++i) {
        const uint64_t a = next(), b = next();
        const int em = (int)(a % 120) - 60, es = (int)((a >> 8) % 60) - 30;
        const float m0 = ldexpf(1.0f + (float)((a >> 16) & 0x7fffff) * 0x1p-23f, em);
        const float sv = ldexpf(1.0f + (float)((b >> 8) & 0x7fffff) * 0x1p-23f, es);
        // av = m0 * sv * (1 + j * 2^-22), j in [-16, 15]: both sides of the threshold 1 - 2^-20, then a few ulp of jitter
        const int j = (int)((b >> 32) & 31) - 16, jit = (int)((b >> 40) & 7) - 3;
        volatile float av0 = m0 * sv;
        volatile float av1 = av0 * (1.0f + (float)j * 0x1p-22f);
        const float av = from_bits((uint32_t)((int64_t)bits(av1) + jit));
        reach(m0, m, thr, nan, p);
        candidate(rnd, av, sv, m, thr, nan, p);
    }

    // ---- special values of sv and av against states of m from 0 through subnormal and normal to inf
    {
        const float ms[] = {0.f, from_bits(1u), from_bits(3u), 0x1p-126f, 0x1p-100f, 1.0f, 3.5f, 0x1.fffffep127f, INFINITY};
        const float svs[] = {0.f, -0.f, from_bits(1u), from_bits(0x007fffffu), 0x1p-126f, 1.0f, 0.5f, -1.0f, -0x1p-140f, INFINITY, -INFINITY, NAN};
        const float avs[] = {0.f, from_bits(1u), 0x1p-126f, 0.25f, 1.0f, 3.5f, 4.0f, 0x1.fffffep127f, INFINITY, NAN};
        for (float m0 : ms)
            for (float sv : svs)
                for (float av : avs) {
                    m = 0.f; thr = 0.f; nan = false; p = Plain();
                    if (m0 != 0.f) reach(m0, m, thr, nan, p);
                    candidate(special, av, sv, m, thr, nan, p);
                    candidate(special, 1.0f, 1.0f, m, thr, nan, p);         // the state it left still works
                }
    }

    int rc = 0;
    for (Regime *r : {&grid, &edge, &rnd, &special}) {
        printf("%-8s skipped %lld divided %lld mismatches %lld\n", r->name, r->skipped, r->divided, r->bad);
        if (r->bad || !r->skipped || !r->divided) rc = 1;
    }
    if (!rc) printf("guarded divide ok\n");
    return rc;
}
