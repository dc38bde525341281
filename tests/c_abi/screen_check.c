/* A C99 client of libcp_pre_screen.so: the wave star screened against three levels on a tiny grid, checked against plain C
 * loops (the definitions of cp_pre_screen.h; Joint/NS_Residuals_CP.py:318-329), two slabs accumulated into one pair of
 * buffers, PRE_FLAG_INTERIOR_T, plus the argument errors the entries return before any device work.  Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/screen_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_screen.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o screen_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_screen.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 2, T = 6, X = 9, Y = 68, N = B * T * X * Y, NK = 3 };

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f - 0.5f; }
static size_t at(int b, int t, int x, int y) { return (((size_t)b * T + t) * X + x) * Y + y; }
static double cell(const float *f, int b, int t, int x, int y)
{
    return (t >= 0 && t < T && x >= 0 && x < X && y >= 0 && y < Y) ? (double)f[at(b, t, x, y)] : 0.0;
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_screen_abi_version() == PRE_SCREEN_ABI_VERSION, "pre_screen_abi_version");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    float *hf = malloc(sizeof(float) * N), *hm = malloc(sizeof(float) * T * X * Y);
    unsigned s = 5u;
    for (int i = 0; i < N; ++i) hf[i] = 1.0f + frand(&s);
    for (int i = 0; i < T * X * Y; ++i) hm[i] = 0.75f + 0.5f * (frand(&s) + 0.5f);
    const float hq[NK] = {0.5f, 1.5f, 100.0f};
    /* an asymmetric 7-point star */
    const float tw[7] = {-1.75f, 0.5f, -1.25f, 0.875f, -0.375f, 1.5f, -0.625f};
    const int32_t toff[21] = {0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1};

    float *df, *dm, *dq;
    uint32_t *dacc;
    CHECK_HIP(hipMalloc((void **)&df, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dm, sizeof(float) * T * X * Y));
    CHECK_HIP(hipMalloc((void **)&dq, sizeof(float) * NK));
    CHECK_HIP(hipMalloc((void **)&dacc, sizeof(uint32_t) * (NK + 1) * B));
    CHECK_HIP(hipMemcpy(df, hf, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dm, hm, sizeof(float) * T * X * Y, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dq, hq, sizeof(float) * NK, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * (NK + 1) * B));

    const int64_t sB = (int64_t)T * X * Y, sT = (int64_t)X * Y, sX = Y;
    pre_field_t f = {df, sB, sT, sX, 1};
    pre_screen_t sc = {dq, NK, dm, sT, sX, 1, 1, 1, dacc, dacc + B, B};

    /* the reference: interior cells, r in double from the fp32 inputs */
    double want_s[B];
    unsigned want_c[NK][B], und[NK][B];
    double rmax = 0.0;
    for (int b = 0; b < B; ++b) {
        want_s[b] = 0.0;
        for (int k = 0; k < NK; ++k) want_c[k][b] = und[k][b] = 0;
    }
    for (int pass = 0; pass < 2; ++pass)
        for (int b = 0; b < B; ++b) for (int t = 1; t < T - 1; ++t) for (int x = 1; x < X - 1; ++x) for (int y = 1; y < Y - 1; ++y) {
            const double r = tw[0] * cell(hf, b, t, x, y) + tw[1] * cell(hf, b, t - 1, x, y) + tw[2] * cell(hf, b, t + 1, x, y) +
                             tw[3] * cell(hf, b, t, x - 1, y) + tw[4] * cell(hf, b, t, x + 1, y) + tw[5] * cell(hf, b, t, x, y - 1) +
                             tw[6] * cell(hf, b, t, x, y + 1);
            const double m = hm[((size_t)t * X + x) * Y + y];
            if (pass == 0) { rmax = fmax(rmax, fabs(r)); continue; }
            want_s[b] = fmax(want_s[b], fabs(r) / m);
            for (int k = 0; k < NK; ++k) {
                const double hw = (double)hq[k] * m;
                if (fabs(r) <= hw) ++want_c[k][b];
                if (fabs(fabs(r) - hw) <= 1e-5 * rmax) ++und[k][b];
            }
        }

    /* the whole grid, then the same grid as two t-slabs with their halo planes into fresh buffers */
    int rc = pre_screen_stencil3d_f32(&f, tw, toff, 7, &sc, B, T, X, Y, 0, NULL);
    EXPECT(rc == PRE_OK, "pre_screen_stencil3d_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    uint32_t whole[(NK + 1) * B], slabs[(NK + 1) * B];
    CHECK_HIP(hipMemcpy(whole, dacc, sizeof(whole), hipMemcpyDeviceToHost));
    int ok_s = 1, ok_c = 1;
    for (int b = 0; b < B; ++b) {
        float got;
        memcpy(&got, &whole[b], sizeof(float));
        printf("      sample %d: score %.7g (C loop %.7g)\n", b, got, want_s[b]);
        if (fabs(got - want_s[b]) > 1e-5 * rmax / 0.75 + 1e-6 * want_s[b]) ok_s = 0;
        for (int k = 0; k < NK; ++k) {
            const long d = (long)whole[(1 + k) * B + b] - (long)want_c[k][b];
            if (labs(d) > (long)und[k][b]) ok_c = 0;
        }
    }
    EXPECT(ok_s, "scores match the C loops (crop, modulation)");
    EXPECT(ok_c, "inside counts match the C loops up to the undecided cells");
    EXPECT(whole[(1 + 2) * B] == (T - 2) * (X - 2) * (Y - 2), "a level above every score holds every counted cell");

    CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * (NK + 1) * B));
    pre_field_t f0 = {df, sB, sT, sX, 1}, f1 = {df + 2 * sT, sB, sT, sX, 1};
    pre_screen_t s0 = sc, s1 = sc;
    s1.modulation = dm + 2 * sT;
    rc = pre_screen_stencil3d_f32(&f0, tw, toff, 7, &s0, B, 4, X, Y, 0, NULL);            /* planes 0..3: counts 1..2 */
    EXPECT(rc == PRE_OK, "first t-slab");
    rc = pre_screen_stencil3d_f32(&f1, tw, toff, 7, &s1, B, 4, X, Y, 0, NULL);            /* planes 2..5: counts 3..4 */
    EXPECT(rc == PRE_OK, "second t-slab");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(slabs, dacc, sizeof(slabs), hipMemcpyDeviceToHost));
    EXPECT(memcmp(whole, slabs, sizeof(whole)) == 0, "two t-slabs accumulate to the bits of the whole grid");

    /* PRE_FLAG_INTERIOR_T: planes 0 and T - 1 neither evaluated nor counted - ct = 0 with the flag is ct = 1 without it */
    CHECK_HIP(hipMemset(dacc, 0, sizeof(uint32_t) * (NK + 1) * B));
    pre_screen_t sf = sc;
    sf.ct = 0;
    rc = pre_screen_stencil3d_f32(&f, tw, toff, 7, &sf, B, T, X, Y, PRE_FLAG_INTERIOR_T, NULL);
    EXPECT(rc == PRE_OK, "PRE_FLAG_INTERIOR_T with ct = 0");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(slabs, dacc, sizeof(slabs), hipMemcpyDeviceToHost));
    EXPECT(memcmp(whole, slabs, sizeof(whole)) == 0, "PRE_FLAG_INTERIOR_T with ct = 0 gives the bits of ct = 1");

    /* ---- argument errors: nothing is launched */
    EXPECT(pre_screen_stencil3d_f32(NULL, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null field -> PRE_E_NULL");
    EXPECT(pre_screen_stencil3d_f32(&f, tw, toff, 7, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null pre_screen_t -> PRE_E_NULL");
    EXPECT(pre_screen_stencil3d_f32(&f, tw, toff, 7, &sc, B, 0, X, Y, 0, NULL) == PRE_E_NULL, "empty extent -> PRE_E_NULL");
    pre_screen_t bad = sc;
    bad.nk = 17;
    EXPECT(pre_screen_stencil3d_f32(&f, tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "17 levels -> PRE_E_RANGE");
    bad = sc;
    bad.cx = -1;
    EXPECT(pre_screen_stencil3d_f32(&f, tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "negative crop -> PRE_E_RANGE");
    const int32_t box[3] = {1, 1, 0};
    EXPECT(pre_screen_stencil3d_f32(&f, tw, box, 1, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "tap off the star -> PRE_E_UNSUPPORTED");
    pre_field_t tfast = {df, sB, 1, (int64_t)T * Y, T};
    EXPECT(pre_screen_stencil3d_f32(&tfast, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "Nt-fastest view -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screen_stencil3d_f32(&f, tw, toff, 7, &sc, B, T, X, Y - 1, 0, NULL) == PRE_E_UNSUPPORTED, "width 67 -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screen_stencil3d_f32(&f, tw, toff, 7, &sc, B, T, X, Y, PRE_FLAG_ABS, NULL) == PRE_E_UNSUPPORTED, "PRE_FLAG_ABS -> PRE_E_UNSUPPORTED");
    float K[27] = {0}, Kbox[27] = {0};
    K[13] = 1.0f; Kbox[0] = 1.0f;
    EXPECT(pre_screen_linear2_f32(&f, &f, K, NULL, 1.0f, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "linear2: null kernel");
    EXPECT(pre_screen_ns_momentum_f32(&f, &f, &f, K, Kbox, K, K, 0.1f, 0.1f, 0.1f, 0.1f, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED,
           "NS: kernel off the star -> PRE_E_UNSUPPORTED");
    pre_field_t six[6] = {f, f, f, f, f, f};
    EXPECT(pre_screen_mhd_f32(4, six, K, K, K, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "mhd: eq 4 -> PRE_E_RANGE");
    CHECK_HIP(hipMemcpy(slabs, dacc, sizeof(slabs), hipMemcpyDeviceToHost));
    EXPECT(memcmp(whole, slabs, sizeof(whole)) == 0, "refused calls changed nothing");
    hipFree(df); hipFree(dm); hipFree(dq); hipFree(dacc);
    free(hf); free(hm);
    return failures ? 1 : 0;
}
