/* A C99 client of libcp_pre_screen1dpair.so: an asymmetric 5-point star and the Burgers residual (its reference tap structure
 * and a general one) on TWO field sets of a tiny [B,Nt,Nx] batch, their difference screened against three levels, in both
 * layouts (Nx-fastest and Nt-fastest), the second set with a row pitch of its own, checked against plain C loops written
 * here (the definitions of cp_pre_screen1dpair.h; Joint/Burgers_Residuals_CP.py:182-187, 217-220), two overlapping slabs of
 * the plane's ROWS accumulated into one pair of buffers, b == a, plus the argument errors the entries return before any
 * device work.  Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/screen1dpair_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_screen1dpair.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o screen1dpair_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_screen1dpair.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

/* PX / PT: the row pitch of the second set, Nx-fastest / Nt-fastest (the first set is dense) */
enum { B = 2, T = 12, X = 24, P = T * X, N = B * P, NK = 3, NA = (NK + 1) * B, PX = X + 4, PT = T + 4,
       NBX = B * T * PX, NBT = B * X * PT };

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

static int run(int op, const float *a, const int64_t sa[3], const float *b, const int64_t sb[3], const pre_screen_t *s,
               int64_t Tn, int64_t Xn)
{
    static const float tw[5] = {-1.75f, 0.5f, -1.25f, 0.875f, -0.375f};
    static const int32_t toff[10] = {0, 0, -1, 0, 1, 0, 0, -1, 0, 1};
    if (op == 0) return pre_screen1dpair_stencil2d_f32(a, sa, b, sb, tw, toff, 5, s, B, Tn, Xn, 0, NULL);
    return pre_screen1dpair_burgers_f32(a, sa, b, sb, op == 1 ? KT : KTG, KX, KXX, DXc, DTc, NUc, C3c, s, B, Tn, Xn, 0, NULL);
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_screen1dpair_abi_version() == PRE_SCREEN1DPAIR_ABI_VERSION, "pre_screen1dpair_abi_version");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    /* truth ha [B][T][X] and prediction hb [B][T][X] (logical); on the device: the truth dense in both layouts, the
     * prediction with pitched rows (PX, PT), the gaps holding NaN */
    float *ha = malloc(sizeof(float) * N), *hb = malloc(sizeof(float) * N), *hat = malloc(sizeof(float) * N);
    float *hbx = malloc(sizeof(float) * NBX), *hbt = malloc(sizeof(float) * NBT), hm[P], hmt[P];
    unsigned sd = 5u;
    for (int i = 0; i < N; ++i) ha[i] = 1.0f + frand(&sd);
    for (int i = 0; i < N; ++i) hb[i] = 1.0f + frand(&sd);
    for (int i = 0; i < P; ++i) hm[i] = 0.75f + 0.5f * (frand(&sd) + 0.5f);
    for (int i = 0; i < NBX; ++i) hbx[i] = NAN;
    for (int i = 0; i < NBT; ++i) hbt[i] = NAN;
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) {
        hat[(size_t)b * P + x * T + t] = ha[(size_t)b * P + t * X + x];
        hbx[((size_t)b * T + t) * PX + x] = hb[(size_t)b * P + t * X + x];
        hbt[((size_t)b * X + x) * PT + t] = hb[(size_t)b * P + t * X + x];
    }
    for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) hmt[x * T + t] = hm[t * X + x];
    const float hq[NK] = {0.5f, 1.5f, 1000.0f};

    float *da, *dat, *dbx, *dbt, *dm, *dmt, *dq;
    uint32_t *dacc;
    CHECK_HIP(hipMalloc((void **)&da, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dat, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dbx, sizeof(float) * NBX));
    CHECK_HIP(hipMalloc((void **)&dbt, sizeof(float) * NBT));
    CHECK_HIP(hipMalloc((void **)&dm, sizeof(float) * P));
    CHECK_HIP(hipMalloc((void **)&dmt, sizeof(float) * P));
    CHECK_HIP(hipMalloc((void **)&dq, sizeof(float) * NK));
    CHECK_HIP(hipMalloc((void **)&dacc, sizeof(uint32_t) * NA));
    CHECK_HIP(hipMemcpy(da, ha, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dat, hat, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dbx, hbx, sizeof(float) * NBX, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dbt, hbt, sizeof(float) * NBT, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dm, hm, sizeof(float) * P, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dmt, hmt, sizeof(float) * P, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dq, hq, sizeof(float) * NK, hipMemcpyHostToDevice));

    /* strides on (B, Nt, Nx): the truth and the prediction in the two layouts */
    const int64_t sax[3] = {P, X, 1}, sat[3] = {P, 1, T}, sbx[3] = {T * PX, PX, 1}, sbt[3] = {X * PT, 1, PT};
    const pre_screen_t scx = {dq, NK, dm, X, 1, 1, 1, 0, dacc, dacc + B, B};
    const pre_screen_t sct = {dq, NK, dmt, 1, T, 1, 1, 0, dacc, dacc + B, B};
    static const char *opname[3] = {"five-point star", "Burgers (reference taps)", "Burgers (general star)"};
    uint32_t whole[NA], got[NA];
    char what[200];

    for (int op = 0; op < 3; ++op) {
        /* the reference: interior cells, d = r(a) - r(b) in double from the fp32 inputs; tau on the two halves */
        double want_s[B], ramax = 0.0, rbmax = 0.0;
        unsigned want_c[NK][B], und[NK][B];
        for (int b = 0; b < B; ++b) {
            want_s[b] = 0.0;
            for (int k = 0; k < NK; ++k) want_c[k][b] = und[k][b] = 0;
        }
        for (int pass = 0; pass < 2; ++pass)
            for (int b = 0; b < B; ++b) for (int t = 1; t < T - 1; ++t) for (int x = 1; x < X - 1; ++x) {
                const double ra = residual(op, ha, b, t, x), rb = residual(op, hb, b, t, x), m = hm[t * X + x];
                if (pass == 0) { ramax = fmax(ramax, fabs(ra)); rbmax = fmax(rbmax, fabs(rb)); continue; }
                const double d = fabs(ra - rb);
                want_s[b] = fmax(want_s[b], d / m);
                for (int k = 0; k < NK; ++k) {
                    const double hw = (double)hq[k] * m;
                    if (d <= hw) ++want_c[k][b];
                    if (fabs(d - hw) <= 1e-5 * (ramax + rbmax)) ++und[k][b];
                }
            }
        const double tau = 1e-5 * (ramax + rbmax);
        for (int layout = 0; layout < 2; ++layout) {
            const float *a = layout ? dat : da, *b_ = layout ? dbt : dbx;
            const int64_t *sa = layout ? sat : sax, *sb = layout ? sbt : sbx;
            const pre_screen_t *sc = layout ? &sct : &scx;
            const char *lname = layout ? "Nt-fastest" : "Nx-fastest";
            CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * NA));
            int rc = run(op, a, sa, b_, sb, sc, T, X);
            snprintf(what, sizeof what, "%s, %s: PRE_OK", opname[op], lname);
            EXPECT(rc == PRE_OK, what);
            CHECK_HIP(hipDeviceSynchronize());
            CHECK_HIP(hipMemcpy(whole, dacc, sizeof(whole), hipMemcpyDeviceToHost));
            int ok_s = 1, ok_c = 1;
            for (int b = 0; b < B; ++b) {
                float sc_;
                memcpy(&sc_, &whole[b], sizeof(float));
                printf("      sample %d: score %.7g (C loop %.7g)\n", b, sc_, want_s[b]);
                if (!(fabs(sc_ - want_s[b]) <= tau / 0.75 + 1.2e-7 * want_s[b])) ok_s = 0;
                for (int k = 0; k < NK; ++k) {
                    const long d = (long)whole[(1 + k) * B + b] - (long)want_c[k][b];
                    if (labs(d) > (long)und[k][b]) ok_c = 0;
                }
            }
            snprintf(what, sizeof what, "%s, %s: scores match the C loops", opname[op], lname);
            EXPECT(ok_s, what);
            snprintf(what, sizeof what, "%s, %s: counts match the C loops up to the undecided cells", opname[op], lname);
            EXPECT(ok_c, what);
            snprintf(what, sizeof what, "%s, %s: a level above every score holds every counted cell", opname[op], lname);
            EXPECT(whole[(1 + 2) * B] == (T - 2) * (X - 2), what);

            /* two overlapping slabs of the plane's ROWS, each with crop 1, every counted cell once.  Nx-fastest the rows
             * are Nt: [0, 8) and [6, 12) count rows 1..6 and 7..10; Nt-fastest they are Nx: [0, 16) and [14, 24) count
             * rows 1..14 and 15..22 (a slab of the contiguous axis would have to keep a multiple of 4) */
            CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * NA));
            pre_screen_t s1 = *sc;
            if (layout == 0) {
                s1.modulation = sc->modulation + 6 * sc->mT;
                rc = run(op, a, sa, b_, sb, sc, 8, X);
                if (rc == PRE_OK) rc = run(op, a + 6 * sa[1], sa, b_ + 6 * sb[1], sb, &s1, 6, X);
            } else {
                s1.modulation = sc->modulation + 14 * sc->mX;
                rc = run(op, a, sa, b_, sb, sc, T, 16);
                if (rc == PRE_OK) rc = run(op, a + 14 * sa[2], sa, b_ + 14 * sb[2], sb, &s1, T, 10);
            }
            CHECK_HIP(hipDeviceSynchronize());
            CHECK_HIP(hipMemcpy(got, dacc, sizeof(got), hipMemcpyDeviceToHost));
            snprintf(what, sizeof what, "%s, %s: two overlapping row slabs accumulate to the bits of the whole", opname[op], lname);
            EXPECT(rc == PRE_OK && memcmp(whole, got, sizeof(whole)) == 0, what);

            /* b == a: every score +0, every counted cell inside at every level */
            CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * NA));
            rc = run(op, a, sa, a, sa, sc, T, X);
            CHECK_HIP(hipDeviceSynchronize());
            CHECK_HIP(hipMemcpy(got, dacc, sizeof(got), hipMemcpyDeviceToHost));
            int zero = rc == PRE_OK;
            for (int b = 0; b < B; ++b) {
                if (got[b] != 0u) zero = 0;
                for (int k = 0; k < NK; ++k) if (got[(1 + k) * B + b] != (T - 2) * (X - 2)) zero = 0;
            }
            snprintf(what, sizeof what, "%s, %s: b == a gives score +0 and every cell inside", opname[op], lname);
            EXPECT(zero, what);
        }
    }

    /* ---- argument errors: nothing is launched.  `whole` / dacc hold the last accumulation */
    CHECK_HIP(hipMemcpy(whole, dacc, sizeof(whole), hipMemcpyDeviceToHost));
    static const float tw[2] = {1.0f, 2.0f};
    static const int32_t on[4] = {0, 0, 0, 1}, corner[4] = {0, 0, 1, 1}, far4[4] = {0, 0, 0, 4};
#define ST2(a, sa, b, sb, w, o, n, s, t, x, fl) pre_screen1dpair_stencil2d_f32(a, sa, b, sb, w, o, n, s, B, t, x, fl, NULL)
#define BG(a, sa, b, sb, kt, kx, kxx, s, t, x, fl) pre_screen1dpair_burgers_f32(a, sa, b, sb, kt, kx, kxx, DXc, DTc, NUc, C3c, s, B, t, x, fl, NULL)
    EXPECT(ST2(NULL, sax, dbx, sbx, tw, on, 2, &scx, T, X, 0) == PRE_E_NULL, "null first set -> PRE_E_NULL");
    EXPECT(ST2(da, sax, NULL, sbx, tw, on, 2, &scx, T, X, 0) == PRE_E_NULL, "null second set -> PRE_E_NULL");
    EXPECT(ST2(da, NULL, dbx, sbx, tw, on, 2, &scx, T, X, 0) == PRE_E_NULL, "null strides of the first set -> PRE_E_NULL");
    EXPECT(ST2(da, sax, dbx, NULL, tw, on, 2, &scx, T, X, 0) == PRE_E_NULL, "null strides of the second set -> PRE_E_NULL");
    EXPECT(ST2(da, sax, dbx, sbx, tw, on, 2, NULL, T, X, 0) == PRE_E_NULL, "null pre_screen_t -> PRE_E_NULL");
    EXPECT(ST2(da, sax, dbx, sbx, NULL, on, 2, &scx, T, X, 0) == PRE_E_NULL, "null tap weights -> PRE_E_NULL");
    EXPECT(ST2(da, sax, dbx, sbx, tw, on, -1, &scx, T, X, 0) == PRE_E_NULL, "negative tap count -> PRE_E_NULL");
    EXPECT(ST2(da, sax, dbx, sbx, tw, on, 2, &scx, 0, X, 0) == PRE_E_NULL, "empty extent -> PRE_E_NULL");
    pre_screen_t bad = scx;
    bad.q = NULL;
    EXPECT(ST2(da, sax, dbx, sbx, tw, on, 2, &bad, T, X, 0) == PRE_E_NULL, "null levels -> PRE_E_NULL");
    bad = scx; bad.count_ld = B - 1;
    EXPECT(ST2(da, sax, dbx, sbx, tw, on, 2, &bad, T, X, 0) == PRE_E_NULL, "count_ld < B -> PRE_E_NULL");
    bad = scx; bad.nk = 17;
    EXPECT(ST2(da, sax, dbx, sbx, tw, on, 2, &bad, T, X, 0) == PRE_E_RANGE, "17 levels -> PRE_E_RANGE");
    bad = scx; bad.cx = -1;
    EXPECT(BG(da, sax, dbx, sbx, KT, KX, KXX, &bad, T, X, 0) == PRE_E_RANGE, "negative crop -> PRE_E_RANGE");
    bad = scx; bad.cy = 1;
    EXPECT(ST2(da, sax, dbx, sbx, tw, on, 2, &bad, T, X, 0) == PRE_E_RANGE, "cy = 1 -> PRE_E_RANGE");
    EXPECT(ST2(da, sax, dbx, sbx, tw, far4, 2, &scx, T, X, 0) == PRE_E_SHAPE, "tap offset 4 -> PRE_E_SHAPE");
    EXPECT(ST2(da, sax, dbx, sbx, tw, corner, 2, &scx, T, X, 0) == PRE_E_UNSUPPORTED, "tap off the star -> PRE_E_UNSUPPORTED");
    EXPECT(ST2(da, sax, dbx, sbx, tw, on, 2, &scx, T, X - 1, 0) == PRE_E_UNSUPPORTED, "width 23 -> PRE_E_UNSUPPORTED");
    EXPECT(BG(dat, sat, dbt, sbt, KT, KX, KXX, &sct, T - 1, X, 0) == PRE_E_UNSUPPORTED, "Nt-fastest with Nt = 11 -> PRE_E_UNSUPPORTED");
    EXPECT(ST2(da, sax, dbt, sbt, tw, on, 2, &scx, T, X, 0) == PRE_E_UNSUPPORTED, "first set Nx-fastest, second Nt-fastest -> PRE_E_UNSUPPORTED");
    EXPECT(BG(dat, sat, dbx, sbx, KT, KX, KXX, &sct, T, X, 0) == PRE_E_UNSUPPORTED, "first set Nt-fastest, second Nx-fastest -> PRE_E_UNSUPPORTED");
    const int64_t s2[3] = {2 * P, 2 * X, 2};
    EXPECT(ST2(da, sax, da, s2, tw, on, 2, &scx, T / 2, X / 2, 0) == PRE_E_UNSUPPORTED, "second set without a unit-stride axis -> PRE_E_UNSUPPORTED");
    EXPECT(ST2(da, sax, dbx, sbx, tw, on, 2, &sct, T, X, 0) == PRE_E_UNSUPPORTED, "sets Nx-fastest, modulation Nt-fastest -> PRE_E_UNSUPPORTED");
    EXPECT(BG(dat, sat, dbt, sbt, KT, KX, KXX, &scx, T, X, 0) == PRE_E_UNSUPPORTED, "sets Nt-fastest, modulation Nx-fastest -> PRE_E_UNSUPPORTED");
    EXPECT(ST2(da, sax, dbx, sbx, tw, on, 2, &scx, T, X, PRE_FLAG_ABS) == PRE_E_UNSUPPORTED, "PRE_FLAG_ABS -> PRE_E_UNSUPPORTED");
    EXPECT(BG(da, sax, dbx, sbx, KT, KX, KXX, &scx, T, X, PRE_FLAG_HALO_X) == PRE_E_UNSUPPORTED, "PRE_FLAG_HALO_X -> PRE_E_UNSUPPORTED");
    EXPECT(BG(da, sax, dbx, sbx, KT, NULL, KXX, &scx, T, X, 0) == PRE_E_NULL, "Burgers: null kernel -> PRE_E_NULL");
    EXPECT(BG(da, sax, NULL, sbx, KT, KX, KXX, &scx, T, X, 0) == PRE_E_NULL, "Burgers: null second set -> PRE_E_NULL");
    float Kc[9] = {0};
    Kc[0] = 1.0f;
    EXPECT(BG(da, sax, dbx, sbx, KT, Kc, KXX, &scx, T, X, 0) == PRE_E_UNSUPPORTED, "Burgers: corner weight -> PRE_E_UNSUPPORTED");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(got, dacc, sizeof(got), hipMemcpyDeviceToHost));
    EXPECT(memcmp(whole, got, sizeof(whole)) == 0, "refused calls changed nothing");
    hipFree(da); hipFree(dat); hipFree(dbx); hipFree(dbt); hipFree(dm); hipFree(dmt); hipFree(dq); hipFree(dacc);
    free(ha); free(hb); free(hat); free(hbx); free(hbt);
    return failures ? 1 : 0;
}
