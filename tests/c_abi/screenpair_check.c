/* A C99 client of libcp_pre_screenpair.so: the wave star on two field sets, d = S(a) - S(b), screened against three levels on
 * a tiny grid in both layouts, checked against plain C loops (the definitions of cp_pre_screenpair.h;
 * Joint/NS_Residuals_CP.py:289-290, 307-313), two t-slabs accumulated into one pair of buffers, b == a giving exactly zero
 * for every entry, plus the argument errors the entries return before any device work.  Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/screenpair_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_screenpair.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o screenpair_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_screenpair.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 2, T = 6, X = 9, Y = 68, P = T * X * Y, N = B * P, NK = 3, ACC = (NK + 1) * B };

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f - 0.5f; }
static size_t at(int b, int t, int x, int y) { return (((size_t)b * T + t) * X + x) * Y + y; }         /* memory [B,T,X,Y] */
static size_t att(int b, int t, int x, int y) { return (((size_t)b * X + x) * Y + y) * T + t; }        /* memory [B,X,Y,T] */
static double cell(const float *f, int b, int t, int x, int y)
{
    return (t >= 0 && t < T && x >= 0 && x < X && y >= 0 && y < Y) ? (double)f[at(b, t, x, y)] : 0.0;
}
static const float tw[7] = {-1.75f, 0.5f, -1.25f, 0.875f, -0.375f, 1.5f, -0.625f};         /* an asymmetric 7-point star */
static const int32_t toff[21] = {0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1};
static double star(const float *f, int b, int t, int x, int y)
{
    return tw[0] * cell(f, b, t, x, y) + tw[1] * cell(f, b, t - 1, x, y) + tw[2] * cell(f, b, t + 1, x, y) +
           tw[3] * cell(f, b, t, x - 1, y) + tw[4] * cell(f, b, t, x + 1, y) + tw[5] * cell(f, b, t, x, y - 1) +
           tw[6] * cell(f, b, t, x, y + 1);
}

/* scores within tol, counts within the undecided cells */
static int agrees(const uint32_t *acc, const double *want_s, unsigned (*want_c)[B], unsigned (*und)[B], double tol)
{
    int ok = 1;
    for (int b = 0; b < B; ++b) {
        float got;
        memcpy(&got, &acc[b], sizeof(float));
        printf("      sample %d: score %.7g (C loop %.7g)\n", b, got, want_s[b]);
        if (fabs(got - want_s[b]) > tol + 1e-6 * want_s[b]) ok = 0;
        for (int k = 0; k < NK; ++k)
            if (labs((long)acc[(1 + k) * B + b] - (long)want_c[k][b]) > (long)und[k][b]) ok = 0;
    }
    return ok;
}

static int all_zero_all_inside(const uint32_t *acc, unsigned cells)
{
    for (int b = 0; b < B; ++b) {
        if (acc[b] != 0u) return 0;
        for (int k = 0; k < NK; ++k)
            if (acc[(1 + k) * B + b] != cells) return 0;
    }
    return 1;
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_screenpair_abi_version() == PRE_SCREENPAIR_ABI_VERSION, "pre_screenpair_abi_version");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    float *ha = malloc(sizeof(float) * N), *hb = malloc(sizeof(float) * N), *hm = malloc(sizeof(float) * P);
    float *hat = malloc(sizeof(float) * N), *hbt = malloc(sizeof(float) * N), *hmt = malloc(sizeof(float) * P);
    unsigned s = 5u;
    for (int i = 0; i < N; ++i) { ha[i] = 1.0f + frand(&s); hb[i] = ha[i] + 0.25f * frand(&s); }
    for (int i = 0; i < P; ++i) hm[i] = 0.75f + 0.5f * (frand(&s) + 0.5f);
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        hat[att(b, t, x, y)] = ha[at(b, t, x, y)];
        hbt[att(b, t, x, y)] = hb[at(b, t, x, y)];
        if (b == 0) hmt[att(0, t, x, y)] = hm[at(0, t, x, y)];
    }
    const float hq[NK] = {0.125f, 0.375f, 100.0f};

    float *da, *db, *dm, *dat, *dbt, *dmt, *dq;
    uint32_t *dacc;
    CHECK_HIP(hipMalloc((void **)&da, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&db, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dat, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dbt, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dm, sizeof(float) * P));
    CHECK_HIP(hipMalloc((void **)&dmt, sizeof(float) * P));
    CHECK_HIP(hipMalloc((void **)&dq, sizeof(float) * NK));
    CHECK_HIP(hipMalloc((void **)&dacc, sizeof(uint32_t) * ACC));
    CHECK_HIP(hipMemcpy(da, ha, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(db, hb, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dat, hat, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dbt, hbt, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dm, hm, sizeof(float) * P, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dmt, hmt, sizeof(float) * P, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dq, hq, sizeof(float) * NK, hipMemcpyHostToDevice));

    const int64_t sB = P, sT = (int64_t)X * Y, sX = Y;
    pre_field_t fa = {da, sB, sT, sX, 1}, fb = {db, sB, sT, sX, 1};
    pre_field_t ta = {dat, sB, 1, (int64_t)Y * T, T}, tb = {dbt, sB, 1, (int64_t)Y * T, T};
    pre_screen_t sc = {dq, NK, dm, sT, sX, 1, 1, 1, dacc, dacc + B, B};
    pre_screenflat_t st = {dq, NK, dmt, 1, (int64_t)Y * T, T, 1, 1, 1, dacc, dacc + B, B};

    /* the reference: interior cells, both residuals in double from the fp32 inputs */
    double want_s[B], ramax = 0.0, rbmax = 0.0;
    unsigned want_c[NK][B], und[NK][B];
    for (int b = 0; b < B; ++b) {
        want_s[b] = 0.0;
        for (int k = 0; k < NK; ++k) want_c[k][b] = und[k][b] = 0;
    }
    for (int pass = 0; pass < 2; ++pass)
        for (int b = 0; b < B; ++b) for (int t = 1; t < T - 1; ++t) for (int x = 1; x < X - 1; ++x) for (int y = 1; y < Y - 1; ++y) {
            const double ra = star(ha, b, t, x, y), rb = star(hb, b, t, x, y), d = fabs(ra - rb);
            const double m = hm[((size_t)t * X + x) * Y + y];
            if (pass == 0) { ramax = fmax(ramax, fabs(ra)); rbmax = fmax(rbmax, fabs(rb)); continue; }
            want_s[b] = fmax(want_s[b], d / m);
            for (int k = 0; k < NK; ++k) {
                const double hw = (double)hq[k] * m;
                if (d <= hw) ++want_c[k][b];
                if (fabs(d - hw) <= 1e-5 * (ramax + rbmax)) ++und[k][b];
            }
        }
    const double tol = 1e-5 * (ramax + rbmax) / 0.75;
    const unsigned cells = (T - 2) * (X - 2) * (Y - 2);
    uint32_t whole[ACC], got[ACC];

    /* ---- Ny-fastest: the whole grid, then two t-slabs with their halo planes */
    CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * ACC));
    int rc = pre_screenpair_stencil3d_f32(&fa, &fb, tw, toff, 7, &sc, B, T, X, Y, 0, NULL);
    EXPECT(rc == PRE_OK, "pre_screenpair_stencil3d_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(whole, dacc, sizeof(whole), hipMemcpyDeviceToHost));
    EXPECT(agrees(whole, want_s, want_c, und, tol), "Ny-fastest: scores and counts match the C loops");
    EXPECT(whole[(1 + 2) * B] == cells, "a level above every score holds every counted cell");

    CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * ACC));
    pre_field_t fa1 = {da + 2 * sT, sB, sT, sX, 1}, fb1 = {db + 2 * sT, sB, sT, sX, 1};
    pre_screen_t s1 = sc;
    s1.modulation = dm + 2 * sT;
    rc = pre_screenpair_stencil3d_f32(&fa, &fb, tw, toff, 7, &sc, B, 4, X, Y, 0, NULL);         /* planes 0..3: counts 1..2 */
    EXPECT(rc == PRE_OK, "first t-slab");
    rc = pre_screenpair_stencil3d_f32(&fa1, &fb1, tw, toff, 7, &s1, B, 4, X, Y, 0, NULL);       /* planes 2..5: counts 3..4 */
    EXPECT(rc == PRE_OK, "second t-slab");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(got, dacc, sizeof(got), hipMemcpyDeviceToHost));
    EXPECT(memcmp(whole, got, sizeof(whole)) == 0, "two t-slabs accumulate to the bits of the whole grid");

    /* ---- Nt-fastest: the same logical tensors with memory [B,X,Y,T] */
    CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * ACC));
    rc = pre_screenpair_flat_stencil3d_f32(&ta, &tb, tw, toff, 7, &st, B, T, X, Y, 0, NULL);
    EXPECT(rc == PRE_OK, "pre_screenpair_flat_stencil3d_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(got, dacc, sizeof(got), hipMemcpyDeviceToHost));
    EXPECT(agrees(got, want_s, want_c, und, tol), "Nt-fastest: scores and counts match the C loops");

    /* ---- b == a: exactly zero, every counted cell inside (q * m > 0), for every entry in both layouts */
    float Kt[27] = {0}, Kx[27] = {0}, Ky[27] = {0}, Kl[27] = {0};
    Kt[4] = -1.0f; Kt[22] = 1.0f;                      /* (t, x, y) = (-1, 0, 0), (1, 0, 0) */
    Kx[10] = -1.0f; Kx[16] = 1.0f;                     /* (0, -1, 0), (0, 1, 0) */
    Ky[12] = -1.0f; Ky[14] = 1.0f;                     /* (0, 0, -1), (0, 0, 1) */
    Kl[10] = Kl[16] = Kl[12] = Kl[14] = 1.0f; Kl[13] = -4.0f;
    float Kyr[27] = {0};                               /* D_y as the reference constructs it: its taps lie along t */
    Kyr[4] = -0.5f; Kyr[22] = 0.5f;
    pre_field_t a3[3] = {fa, fb, fa}, t3[3] = {ta, tb, ta};
    for (int e = 0; e < 8; ++e) {
        static const char *names[8] = {"stencil3d: b == a gives exactly 0", "linear2: b == a gives exactly 0",
                                       "ns_momentum: b == a gives exactly 0", "mhd_continuity: b == a gives exactly 0",
                                       "flat stencil3d: b == a gives exactly 0", "flat linear2: b == a gives exactly 0",
                                       "flat ns_momentum: b == a gives exactly 0", "flat mhd_continuity: b == a gives exactly 0"};
        CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * ACC));
        switch (e) {
        case 0: rc = pre_screenpair_stencil3d_f32(&fa, &fa, tw, toff, 7, &sc, B, T, X, Y, 0, NULL); break;
        case 1: rc = pre_screenpair_linear2_f32(a3, a3, Kx, Ky, 0.5f, &sc, B, T, X, Y, 0, NULL); break;
        case 2: rc = pre_screenpair_ns_momentum_f32(a3, a3, Kt, Kx, Ky, Kl, 0.01f, 0.02f, 0.03f, 0.001f, &sc, B, T, X, Y, 0, NULL); break;
        case 3: rc = pre_screenpair_mhd_continuity_f32(a3, a3, Kt, Kx, Ky, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL); break;
        case 4: rc = pre_screenpair_flat_stencil3d_f32(&ta, &ta, tw, toff, 7, &st, B, T, X, Y, 0, NULL); break;
        case 5: rc = pre_screenpair_flat_linear2_f32(t3, t3, Kx, Ky, 0.5f, &st, B, T, X, Y, 0, NULL); break;
        case 6: rc = pre_screenpair_flat_ns_momentum_f32(t3, t3, Kt, Kx, Kyr, Kl, 0.01f, 0.02f, 0.03f, 0.001f, &st, B, T, X, Y, 0, NULL); break;
        default: rc = pre_screenpair_flat_mhd_continuity_f32(t3, t3, Kt, Kx, Ky, 5.0 / 3.0, &st, B, T, X, Y, 0, NULL); break;
        }
        CHECK_HIP(hipDeviceSynchronize());
        CHECK_HIP(hipMemcpy(got, dacc, sizeof(got), hipMemcpyDeviceToHost));
        EXPECT(rc == PRE_OK && all_zero_all_inside(got, cells), names[e]);
    }

    /* ---- argument errors: nothing is launched */
    CHECK_HIP(hipMemcpy(dacc, whole, sizeof(whole), hipMemcpyHostToDevice));
    EXPECT(pre_screenpair_stencil3d_f32(NULL, &fb, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null first set -> PRE_E_NULL");
    EXPECT(pre_screenpair_stencil3d_f32(&fa, NULL, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null second set -> PRE_E_NULL");
    EXPECT(pre_screenpair_stencil3d_f32(&fa, &fb, tw, toff, 7, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null pre_screen_t -> PRE_E_NULL");
    EXPECT(pre_screenpair_flat_stencil3d_f32(&ta, &tb, tw, toff, 7, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null pre_screenflat_t -> PRE_E_NULL");
    EXPECT(pre_screenpair_linear2_f32(a3, NULL, Kx, Ky, 1.0f, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "linear2: null second set");
    EXPECT(pre_screenpair_ns_momentum_f32(a3, a3, Kt, Kx, NULL, Kl, 0.1f, 0.1f, 0.1f, 0.1f, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "NS: null kernel");
    EXPECT(pre_screenpair_stencil3d_f32(&fa, &fb, tw, toff, 7, &sc, B, 0, X, Y, 0, NULL) == PRE_E_NULL, "empty extent -> PRE_E_NULL");
    pre_screen_t bad = sc;
    bad.nk = 17;
    EXPECT(pre_screenpair_stencil3d_f32(&fa, &fb, tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "17 levels -> PRE_E_RANGE");
    bad = sc;
    bad.cx = -1;
    EXPECT(pre_screenpair_mhd_continuity_f32(a3, a3, Kt, Kx, Ky, 5.0 / 3.0, &bad, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "negative crop -> PRE_E_RANGE");
    const int32_t box[3] = {1, 1, 0};
    EXPECT(pre_screenpair_stencil3d_f32(&fa, &fb, tw, box, 1, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "tap off the star -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenpair_stencil3d_f32(&fa, &tb, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "second set Nt-fastest -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenpair_flat_stencil3d_f32(&ta, &fb, tw, toff, 7, &st, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "flat: second set Ny-fastest -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenpair_stencil3d_f32(&fa, &fb, tw, toff, 7, &sc, B, T, X, Y - 1, 0, NULL) == PRE_E_UNSUPPORTED, "width 67 -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenpair_stencil3d_f32(&fa, &fb, tw, toff, 7, &sc, B, T, X, Y, PRE_FLAG_ABS, NULL) == PRE_E_UNSUPPORTED, "PRE_FLAG_ABS -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenpair_flat_linear2_f32(t3, t3, Kx, Ky, 1.0f, &st, B, T, X, Y, PRE_FLAG_HALO_X, NULL) == PRE_E_UNSUPPORTED, "flat: PRE_FLAG_HALO_X -> PRE_E_UNSUPPORTED");
    float Kbox[27] = {0}, Kgen[27] = {0};
    Kbox[0] = 1.0f;
    Kgen[4] = Kgen[10] = Kgen[12] = 1.0f;              /* a star with weight on all three axes: the general star */
    EXPECT(pre_screenpair_ns_momentum_f32(a3, a3, Kt, Kbox, Ky, Kl, 0.1f, 0.1f, 0.1f, 0.1f, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED,
           "NS: kernel off the star -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenpair_ns_momentum_f32(a3, a3, Kt, Kgen, Ky, Kl, 0.1f, 0.1f, 0.1f, 0.1f, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED,
           "NS: the general star -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenpair_flat_mhd_continuity_f32(t3, t3, Kt, Kgen, Ky, 5.0 / 3.0, &st, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED,
           "flat MHD continuity: the general star -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenpair_flat_ns_momentum_f32(t3, t3, Kt, Kx, Ky, Kl, 0.01f, 0.02f, 0.03f, 0.001f, &st, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED,
           "flat NS momentum: the y-fixed tap structure is not built -> PRE_E_UNSUPPORTED");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(got, dacc, sizeof(got), hipMemcpyDeviceToHost));
    EXPECT(memcmp(whole, got, sizeof(whole)) == 0, "refused calls changed nothing");
    hipFree(da); hipFree(db); hipFree(dat); hipFree(dbt); hipFree(dm); hipFree(dmt); hipFree(dq); hipFree(dacc);
    free(ha); free(hb); free(hm); free(hat); free(hbt); free(hmt);
    return failures ? 1 : 0;
}
