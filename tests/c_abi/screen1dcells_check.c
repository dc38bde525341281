/* A C99 client of libcp_pre_screen1dcells.so: an asymmetric 5-point star and the Burgers residual (its reference tap
 * structure and a general one) on one field set and on a pair of field sets of a tiny [B,Nt,Nx] batch, screened against
 * three PER-CELL level fields, in both layouts (Nx-fastest and Nt-fastest), checked against plain C loops written here (the
 * definitions of cp_pre_screen1dcells.h; Marginal/Burgers_Residuals_CP.py:249-259, 274-283).  B is one more than the sample
 * group of the build, so the last group is partial.  One run without a modulation, two overlapping slabs of the plane's ROWS
 * accumulated into one pair of buffers, b == a, plus the argument errors the entries return before any device work.  Exit
 * code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/screen1dcells_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_screen1dcells.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o screen1dcells_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_screen1dcells.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

/* LK: the level stride, a gap of 8 floats (NaN) after each level field */
enum { T = 12, X = 24, P = T * X, NK = 3, LK = P + 8 };

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f - 0.5f; }
static double cell(const float *f, int b, int t, int x)
{
    return (t >= 0 && t < T && x >= 0 && x < X) ? (double)f[((size_t)b * T + t) * X + x] : 0.0;
}
/* a 3x3 kernel K[a][c] (a over Nt, c over Nx) applied at (t, x) with zero padding */
static double conv9(const float *K, const float *f, int b, int t, int x)
{
    double r = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) r += (double)K[a * 3 + c] * cell(f, b, t + a - 1, x + c - 1);
    return r;
}

static const float KS[9] = {0.f, 0.5f, 0.f, 0.875f, -1.75f, -0.375f, 0.f, -1.25f, 0.f};
static const float KT[9] = {0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
static const float KX[9] = {0.f, 0.f, 0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f};
static const float KXX[9] = {0.f, 0.f, 0.f, 1.f, -2.f, 1.f, 0.f, 0.f, 0.f};
static const float KTG[9] = {0.f, -1.f, 0.f, 0.25f, 0.5f, 0.f, 0.f, 1.f, 0.f};     /* D_t with taps along Nx too: the general star */
static const float DXc = 0.015625f, DTc = 0.01f, NUc = 0.002f, C3c = 1.28f;

static double residual(int op, const float *f, int b, int t, int x)
{
    if (op == 0) return conv9(KS, f, b, t, x);
    const float *kt = op == 1 ? KT : KTG;
    return (double)DXc * conv9(kt, f, b, t, x) + (double)DTc * cell(f, b, t, x) * conv9(KX, f, b, t, x) -
           (double)NUc * conv9(KXX, f, b, t, x) * (double)C3c;
}

static int64_t Bn;       /* samples: the sample group of the build + 1 */

/* b == NULL: the one-set entries */
static int run(int op, const float *a, const int64_t sa[3], const float *b, const int64_t sb[3], const pre_screen1dcells_t *s,
               int64_t Tn, int64_t Xn)
{
    static const float tw[5] = {-1.75f, 0.5f, -1.25f, 0.875f, -0.375f};
    static const int32_t toff[10] = {0, 0, -1, 0, 1, 0, 0, -1, 0, 1};
    const float *kt = op == 1 ? KT : KTG;
    if (!b) {
        if (op == 0) return pre_screen1dcells_stencil2d_f32(a, sa, tw, toff, 5, s, Bn, Tn, Xn, 0, NULL);
        return pre_screen1dcells_burgers_f32(a, sa, kt, KX, KXX, DXc, DTc, NUc, C3c, s, Bn, Tn, Xn, 0, NULL);
    }
    if (op == 0) return pre_screen1dcells_pair_stencil2d_f32(a, sa, b, sb, tw, toff, 5, s, Bn, Tn, Xn, 0, NULL);
    return pre_screen1dcells_pair_burgers_f32(a, sa, b, sb, kt, KX, KXX, DXc, DTc, NUc, C3c, s, Bn, Tn, Xn, 0, NULL);
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_screen1dcells_abi_version() == PRE_SCREEN1DCELLS_ABI_VERSION, "pre_screen1dcells_abi_version");
    const int G = pre_screen1dcells_sample_group();
    EXPECT(G >= 1, "pre_screen1dcells_sample_group >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    Bn = G + 1;
    const int B = (int)Bn;
    const size_t N = (size_t)B * P, NA = (size_t)(NK + 1) * B;
    /* the two sets ha, hb [B][T][X] (logical) and their Nt-fastest copies; the modulation; the level fields of an op are
     * made below from its residuals */
    float *ha = malloc(sizeof(float) * N), *hb = malloc(sizeof(float) * N), *hat = malloc(sizeof(float) * N);
    float *hbt = malloc(sizeof(float) * N), hm[P], hmt[P], hu[P], hq[NK * LK], hqt[NK * LK];
    uint32_t *whole = malloc(sizeof(uint32_t) * NA), *got = malloc(sizeof(uint32_t) * NA);
    double *want_s = malloc(sizeof(double) * B);
    unsigned *want_c = malloc(sizeof(unsigned) * NK * B), *und = malloc(sizeof(unsigned) * NK * B);
    unsigned sd = 5u;
    for (size_t i = 0; i < N; ++i) ha[i] = 1.0f + frand(&sd);
    for (size_t i = 0; i < N; ++i) hb[i] = ha[i] + 0.25f * frand(&sd);
    for (int i = 0; i < P; ++i) hm[i] = 0.75f + 0.5f * (frand(&sd) + 0.5f);
    for (int i = 0; i < P; ++i) hu[i] = 0.5f + (frand(&sd) + 0.5f);
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) {
        hat[(size_t)b * P + x * T + t] = ha[(size_t)b * P + t * X + x];
        hbt[(size_t)b * P + x * T + t] = hb[(size_t)b * P + t * X + x];
    }
    for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) hmt[x * T + t] = hm[t * X + x];

    float *da, *dat, *db, *dbt, *dm, *dmt, *dq, *dqt;
    uint32_t *dacc;
    CHECK_HIP(hipMalloc((void **)&da, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dat, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&db, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dbt, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dm, sizeof(float) * P));
    CHECK_HIP(hipMalloc((void **)&dmt, sizeof(float) * P));
    CHECK_HIP(hipMalloc((void **)&dq, sizeof(hq)));
    CHECK_HIP(hipMalloc((void **)&dqt, sizeof(hqt)));
    CHECK_HIP(hipMalloc((void **)&dacc, sizeof(uint32_t) * NA));
    CHECK_HIP(hipMemcpy(da, ha, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dat, hat, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(db, hb, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dbt, hbt, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dm, hm, sizeof(float) * P, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dmt, hmt, sizeof(float) * P, hipMemcpyHostToDevice));

    /* strides on (B, Nt, Nx) in the two layouts; the descriptors: crop 1 on both axes */
    const int64_t sx[3] = {P, X, 1}, st[3] = {P, 1, T};
    const pre_screen1dcells_t scx = {dq, NK, LK, X, 1, dm, X, 1, 1, 1, dacc, dacc + B, B};
    const pre_screen1dcells_t sct = {dqt, NK, LK, 1, T, dmt, 1, T, 1, 1, dacc, dacc + B, B};
    static const char *opname[3] = {"five-point star", "Burgers (reference taps)", "Burgers (general star)"};
    static const float lev[NK] = {0.5f, 1.5f, 1000.0f};
    const unsigned counted = (T - 2) * (X - 2);
    char what[240];

    for (int op = 0; op < 3; ++op) for (int pair = 0; pair < 2; ++pair) for (int mod = 1; mod >= 0; --mod) {
        if (!mod && (op != 0 || pair)) continue;          /* once without a modulation: the star on one set */
        /* the reference: interior cells, r (or d = r(a) - r(b)) in double from the fp32 inputs; the level fields are
         * lev[k] * hu[cell] * mean |r|, so the first two split a sample's cells and the third holds them all */
        double rmax = 0.0, rsum = 0.0;
        for (int b = 0; b < B; ++b) for (int t = 1; t < T - 1; ++t) for (int x = 1; x < X - 1; ++x) {
            const double ra = residual(op, ha, b, t, x), rb = pair ? residual(op, hb, b, t, x) : 0.0;
            rmax = fmax(rmax, fabs(ra) + fabs(rb));
            rsum += fabs(ra - rb);
        }
        const double tau = 1e-5 * rmax, mean = rsum / ((double)B * counted);
        for (int i = 0; i < NK * LK; ++i) hq[i] = hqt[i] = NAN;
        for (int k = 0; k < NK; ++k) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x)
            hqt[k * LK + x * T + t] = hq[k * LK + t * X + x] = (float)(lev[k] * hu[t * X + x] * mean);
        CHECK_HIP(hipMemcpy(dq, hq, sizeof(hq), hipMemcpyHostToDevice));
        CHECK_HIP(hipMemcpy(dqt, hqt, sizeof(hqt), hipMemcpyHostToDevice));
        for (int b = 0; b < B; ++b) {
            want_s[b] = 0.0;
            for (int k = 0; k < NK; ++k) want_c[k * B + b] = und[k * B + b] = 0;
            for (int t = 1; t < T - 1; ++t) for (int x = 1; x < X - 1; ++x) {
                const double d = fabs(residual(op, ha, b, t, x) - (pair ? residual(op, hb, b, t, x) : 0.0));
                const float m = mod ? hm[t * X + x] : 1.0f;
                want_s[b] = fmax(want_s[b], d / m);
                for (int k = 0; k < NK; ++k) {
                    const double hw = (double)(float)(hq[k * LK + t * X + x] * m);      /* one fp32 product */
                    if (d <= hw) ++want_c[k * B + b];
                    if (fabs(d - hw) <= tau) ++und[k * B + b];
                }
            }
        }
        for (int layout = 0; layout < 2; ++layout) {
            const float *a = layout ? dat : da, *b_ = pair ? (layout ? dbt : db) : NULL;
            const int64_t *sa = layout ? st : sx;
            pre_screen1dcells_t sc = layout ? sct : scx;
            if (!mod) sc.modulation = NULL;
            snprintf(what, sizeof what, "%s%s%s, %s", opname[op], pair ? ", pair" : "", mod ? "" : ", no modulation",
                     layout ? "Nt-fastest" : "Nx-fastest");
            const size_t w0 = strlen(what);
            CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * NA));
            int rc = run(op, a, sa, b_, sa, &sc, T, X);
            snprintf(what + w0, sizeof what - w0, ": PRE_OK");
            EXPECT(rc == PRE_OK, what);
            CHECK_HIP(hipDeviceSynchronize());
            CHECK_HIP(hipMemcpy(whole, dacc, sizeof(uint32_t) * NA, hipMemcpyDeviceToHost));
            int ok_s = 1, ok_c = 1, ok_all = 1;
            for (int b = 0; b < B; ++b) {
                float sc_;
                memcpy(&sc_, &whole[b], sizeof(float));
                if (b < 2 || b == B - 1) printf("      sample %d: score %.7g (C loop %.7g)\n", b, sc_, want_s[b]);
                if (!(fabs(sc_ - want_s[b]) <= tau / 0.75 + 1.2e-7 * want_s[b])) ok_s = 0;
                for (int k = 0; k < NK; ++k) {
                    const long d = (long)whole[(size_t)(1 + k) * B + b] - (long)want_c[k * B + b];
                    if (labs(d) > (long)und[k * B + b]) ok_c = 0;
                }
                if (whole[(size_t)(1 + 2) * B + b] != counted) ok_all = 0;
            }
            snprintf(what + w0, sizeof what - w0, ": scores match the C loops");
            EXPECT(ok_s, what);
            snprintf(what + w0, sizeof what - w0, ": counts match the C loops up to the undecided cells");
            EXPECT(ok_c, what);
            snprintf(what + w0, sizeof what - w0, ": level fields above every score hold every counted cell of every sample");
            EXPECT(ok_all, what);
            if (!mod) continue;

            /* two overlapping slabs of the plane's ROWS, each with crop 1, every counted cell once.  Nx-fastest the rows
             * are Nt: [0, 8) and [6, 12) count rows 1..6 and 7..10; Nt-fastest they are Nx: [0, 16) and [14, 24) count
             * rows 1..14 and 15..22.  The modulation and the level fields of the second slab start at its first row */
            CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * NA));
            pre_screen1dcells_t s1 = sc;
            if (layout == 0) {
                s1.modulation = sc.modulation + 6 * sc.mT;
                s1.levels = sc.levels + 6 * sc.lT;
                rc = run(op, a, sa, b_, sa, &sc, 8, X);
                if (rc == PRE_OK) rc = run(op, a + 6 * sa[1], sa, b_ ? b_ + 6 * sa[1] : NULL, sa, &s1, 6, X);
            } else {
                s1.modulation = sc.modulation + 14 * sc.mX;
                s1.levels = sc.levels + 14 * sc.lX;
                rc = run(op, a, sa, b_, sa, &sc, T, 16);
                if (rc == PRE_OK) rc = run(op, a + 14 * sa[2], sa, b_ ? b_ + 14 * sa[2] : NULL, sa, &s1, T, 10);
            }
            CHECK_HIP(hipDeviceSynchronize());
            CHECK_HIP(hipMemcpy(got, dacc, sizeof(uint32_t) * NA, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < NA; ++i)
                if (whole[i] != got[i])
                    printf("      %s of sample %d: whole 0x%08x, slabs 0x%08x\n", i < (size_t)B ? "score" : "count", (int)(i % B),
                           (unsigned)whole[i], (unsigned)got[i]);
            snprintf(what + w0, sizeof what - w0, ": two overlapping row slabs accumulate to the bits of the whole");
            EXPECT(rc == PRE_OK && memcmp(whole, got, sizeof(uint32_t) * NA) == 0, what);
            if (!pair) continue;

            /* b == a: every score +0, every counted cell inside at every (positive) level */
            CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * NA));
            rc = run(op, a, sa, a, sa, &sc, T, X);
            CHECK_HIP(hipDeviceSynchronize());
            CHECK_HIP(hipMemcpy(got, dacc, sizeof(uint32_t) * NA, hipMemcpyDeviceToHost));
            int zero = rc == PRE_OK;
            for (int b = 0; b < B; ++b) {
                if (got[b] != 0u) zero = 0;
                for (int k = 0; k < NK; ++k) if (got[(size_t)(1 + k) * B + b] != counted) zero = 0;
            }
            snprintf(what + w0, sizeof what - w0, ": b == a gives score +0 and every cell inside");
            EXPECT(zero, what);
        }
    }

    /* ---- argument errors: nothing is launched.  `whole` / dacc hold the last accumulation */
    CHECK_HIP(hipMemcpy(whole, dacc, sizeof(uint32_t) * NA, hipMemcpyDeviceToHost));
    static const float tw[2] = {1.0f, 2.0f};
    static const int32_t on[4] = {0, 0, 0, 1}, corner[4] = {0, 0, 1, 1}, far4[4] = {0, 0, 0, 4};
#define ST1(a, sa, w, o, n, s, t, x, fl) pre_screen1dcells_stencil2d_f32(a, sa, w, o, n, s, Bn, t, x, fl, NULL)
#define BG1(a, sa, kt, kx, kxx, s, t, x, fl) pre_screen1dcells_burgers_f32(a, sa, kt, kx, kxx, DXc, DTc, NUc, C3c, s, Bn, t, x, fl, NULL)
#define ST2(a, sa, b, sb, w, o, n, s, t, x, fl) pre_screen1dcells_pair_stencil2d_f32(a, sa, b, sb, w, o, n, s, Bn, t, x, fl, NULL)
#define BG2(a, sa, b, sb, kt, kx, kxx, s, t, x, fl) pre_screen1dcells_pair_burgers_f32(a, sa, b, sb, kt, kx, kxx, DXc, DTc, NUc, C3c, s, Bn, t, x, fl, NULL)
    EXPECT(ST1(NULL, sx, tw, on, 2, &scx, T, X, 0) == PRE_E_NULL, "null field -> PRE_E_NULL");
    EXPECT(ST1(da, NULL, tw, on, 2, &scx, T, X, 0) == PRE_E_NULL, "null strides -> PRE_E_NULL");
    EXPECT(ST2(da, sx, NULL, sx, tw, on, 2, &scx, T, X, 0) == PRE_E_NULL, "null second set -> PRE_E_NULL");
    EXPECT(BG2(da, sx, db, NULL, KT, KX, KXX, &scx, T, X, 0) == PRE_E_NULL, "null strides of the second set -> PRE_E_NULL");
    EXPECT(ST1(da, sx, tw, on, 2, NULL, T, X, 0) == PRE_E_NULL, "null descriptor -> PRE_E_NULL");
    EXPECT(ST1(da, sx, NULL, on, 2, &scx, T, X, 0) == PRE_E_NULL, "null tap weights -> PRE_E_NULL");
    EXPECT(ST1(da, sx, tw, on, -1, &scx, T, X, 0) == PRE_E_NULL, "negative tap count -> PRE_E_NULL");
    EXPECT(ST1(da, sx, tw, on, 2, &scx, 0, X, 0) == PRE_E_NULL, "empty extent -> PRE_E_NULL");
    pre_screen1dcells_t bad = scx;
    bad.levels = NULL;
    EXPECT(ST1(da, sx, tw, on, 2, &bad, T, X, 0) == PRE_E_NULL, "null levels -> PRE_E_NULL");
    bad = scx; bad.count_ld = B - 1;
    EXPECT(BG1(da, sx, KT, KX, KXX, &bad, T, X, 0) == PRE_E_NULL, "count_ld < B -> PRE_E_NULL");
    bad = scx; bad.nk = 17;
    EXPECT(ST1(da, sx, tw, on, 2, &bad, T, X, 0) == PRE_E_RANGE, "17 levels -> PRE_E_RANGE");
    bad = scx; bad.cx = -1;
    EXPECT(BG1(da, sx, KT, KX, KXX, &bad, T, X, 0) == PRE_E_RANGE, "negative crop -> PRE_E_RANGE");
    bad = scx; bad.lK = -1;
    EXPECT(ST1(da, sx, tw, on, 2, &bad, T, X, 0) == PRE_E_SHAPE, "negative level stride -> PRE_E_SHAPE");
    bad = scx; bad.lT = -X;
    EXPECT(BG2(da, sx, db, sx, KT, KX, KXX, &bad, T, X, 0) == PRE_E_SHAPE, "negative row stride of the levels -> PRE_E_SHAPE");
    bad = scx; bad.lK = 0;
    EXPECT(ST1(da, sx, tw, on, 2, &bad, T, X, PRE_FLAG_ABS) == PRE_E_UNSUPPORTED, "PRE_FLAG_ABS -> PRE_E_UNSUPPORTED");
    EXPECT(ST1(da, sx, tw, far4, 2, &scx, T, X, 0) == PRE_E_SHAPE, "tap offset 4 -> PRE_E_SHAPE");
    EXPECT(ST1(da, sx, tw, corner, 2, &scx, T, X, 0) == PRE_E_UNSUPPORTED, "tap off the star -> PRE_E_UNSUPPORTED");
    EXPECT(ST1(da, sx, tw, on, 2, &scx, T, X - 1, 0) == PRE_E_UNSUPPORTED, "width 23 -> PRE_E_UNSUPPORTED");
    EXPECT(BG1(dat, st, KT, KX, KXX, &sct, T - 1, X, 0) == PRE_E_UNSUPPORTED, "Nt-fastest with Nt = 11 -> PRE_E_UNSUPPORTED");
    EXPECT(ST2(da, sx, dbt, st, tw, on, 2, &scx, T, X, 0) == PRE_E_UNSUPPORTED, "first set Nx-fastest, second Nt-fastest -> PRE_E_UNSUPPORTED");
    EXPECT(ST1(da, sx, tw, on, 2, &sct, T, X, 0) == PRE_E_UNSUPPORTED, "field Nx-fastest, modulation and levels Nt-fastest -> PRE_E_UNSUPPORTED");
    bad = scx; bad.lT = 1; bad.lX = T;
    EXPECT(ST1(da, sx, tw, on, 2, &bad, T, X, 0) == PRE_E_UNSUPPORTED, "field and modulation Nx-fastest, levels Nt-fastest -> PRE_E_UNSUPPORTED");
    bad = sct; bad.lT = X; bad.lX = 1;
    EXPECT(BG2(dat, st, dbt, st, KT, KX, KXX, &bad, T, X, 0) == PRE_E_UNSUPPORTED, "sets and modulation Nt-fastest, levels Nx-fastest -> PRE_E_UNSUPPORTED");
    bad = scx; bad.lX = 2;
    EXPECT(ST1(da, sx, tw, on, 2, &bad, T, X, 0) == PRE_E_UNSUPPORTED, "levels without a unit-stride axis -> PRE_E_UNSUPPORTED");
    EXPECT(BG1(da, sx, KT, KX, KXX, &scx, T, X, PRE_FLAG_HALO_X) == PRE_E_UNSUPPORTED, "PRE_FLAG_HALO_X -> PRE_E_UNSUPPORTED");
    EXPECT(BG1(da, sx, KT, NULL, KXX, &scx, T, X, 0) == PRE_E_NULL, "Burgers: null kernel -> PRE_E_NULL");
    float Kc[9] = {0};
    Kc[0] = 1.0f;
    EXPECT(BG1(da, sx, KT, Kc, KXX, &scx, T, X, 0) == PRE_E_UNSUPPORTED, "Burgers: corner weight -> PRE_E_UNSUPPORTED");
    EXPECT(BG2(da, sx, db, sx, KT, Kc, KXX, &scx, T, X, 0) == PRE_E_UNSUPPORTED, "paired Burgers: corner weight -> PRE_E_UNSUPPORTED");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(got, dacc, sizeof(uint32_t) * NA, hipMemcpyDeviceToHost));
    EXPECT(memcmp(whole, got, sizeof(uint32_t) * NA) == 0, "refused calls changed nothing");
    hipFree(da); hipFree(dat); hipFree(db); hipFree(dbt); hipFree(dm); hipFree(dmt); hipFree(dq); hipFree(dqt); hipFree(dacc);
    free(ha); free(hb); free(hat); free(hbt); free(whole); free(got); free(want_s); free(want_c); free(und);
    return failures ? 1 : 0;
}
