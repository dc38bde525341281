/* A C99 client of libcp_pre_screencellspair.so: the difference d = S(a) - S(b) of a star applied to two field sets, screened
 * against three per-cell level fields on a tiny grid, in both forms (Ny-fastest and Nt-fastest memory), with one sample more
 * than a sample group, checked against plain C loops (the definitions of cp_pre_screencellspair.h;
 * Marginal/Wave_Residuals_CP.py:219-254), two t-slabs accumulated into one pair of buffers, b == a, plus the argument errors
 * the entries return before any device work.  Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/screencellspair_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_screencellspair.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o screencellspair_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_screencellspair.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { T = 6, X = 9, Y = 68, P = T * X * Y, NK = 3, BMAX = 80 };
static int B;

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f - 0.5f; }
static size_t at(int b, int t, int x, int y) { return (((size_t)b * T + t) * X + x) * Y + y; }
static size_t pat(int t, int x, int y) { return ((size_t)t * X + x) * Y + y; }
static size_t fat(int t, int x, int y) { return ((size_t)x * Y + y) * T + t; }      /* a plane cell in memory [X,Y,T] */
static double cell(const float *f, int b, int t, int x, int y)
{
    return (t >= 0 && t < T && x >= 0 && x < X && y >= 0 && y < Y) ? (double)f[at(b, t, x, y)] : 0.0;
}

/* compare accumulators [NK+1][B] with the C loops */
static int matches(const uint32_t *acc, const double *want_s, const unsigned *want_c, const unsigned *und, double rmax)      /* rmax: max |S(a)| + max |S(b)| */
{
    int ok = 1;
    for (int b = 0; b < B; ++b) {
        float got;
        memcpy(&got, &acc[b], sizeof(float));
        if (fabs(got - want_s[b]) > 1e-5 * rmax / 0.75 + 1e-6 * want_s[b]) ok = 0;
        for (int k = 0; k < NK; ++k) {
            const long d = (long)acc[(1 + k) * B + b] - (long)want_c[k * B + b];
            if (labs(d) > (long)und[k * B + b]) ok = 0;
        }
    }
    return ok;
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_screencellspair_abi_version() == PRE_SCREENCELLSPAIR_ABI_VERSION, "pre_screencellspair_abi_version");
    const int G = pre_screencellspair_sample_group();
    EXPECT(G >= 1, "pre_screencellspair_sample_group >= 1");
    B = G + 1 <= BMAX ? G + 1 : BMAX;                     /* one sample in the last group */
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    const size_t N = (size_t)B * P;
    float *hf = malloc(sizeof(float) * N), *hff = malloc(sizeof(float) * N), *hg = malloc(sizeof(float) * N),
          *hgf = malloc(sizeof(float) * N), *hm = malloc(sizeof(float) * P),
          *hmf = malloc(sizeof(float) * P), *hq = malloc(sizeof(float) * NK * P), *hqf = malloc(sizeof(float) * NK * P);
    unsigned s = 5u;
    const float base[NK] = {0.1f, 0.3f, 100.0f};
    for (size_t i = 0; i < N; ++i) hf[i] = 1.0f + frand(&s);
    for (size_t i = 0; i < N; ++i) hg[i] = hf[i] + 0.25f * frand(&s);          /* the prediction: the truth and an error */
    for (int i = 0; i < P; ++i) hm[i] = 0.75f + 0.5f * (frand(&s) + 0.5f);
    for (int k = 0; k < NK; ++k)
        for (int i = 0; i < P; ++i) hq[k * P + i] = base[k] * (1.0f + frand(&s));
    /* the same tensors with memory [B,X,Y,T] / [X,Y,T] / [NK,X,Y,T] */
    for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        for (int b = 0; b < B; ++b) hff[(size_t)b * P + fat(t, x, y)] = hf[at(b, t, x, y)];
        for (int b = 0; b < B; ++b) hgf[(size_t)b * P + fat(t, x, y)] = hg[at(b, t, x, y)];
        hmf[fat(t, x, y)] = hm[pat(t, x, y)];
        for (int k = 0; k < NK; ++k) hqf[(size_t)k * P + fat(t, x, y)] = hq[(size_t)k * P + pat(t, x, y)];
    }
    /* an asymmetric 7-point star */
    const float tw[7] = {-1.75f, 0.5f, -1.25f, 0.875f, -0.375f, 1.5f, -0.625f};
    const int32_t toff[21] = {0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1};

    float *df, *dff, *dg, *dgf, *dm, *dmf, *dq, *dqf;
    uint32_t *dacc;
    const size_t accb = sizeof(uint32_t) * (NK + 1) * B;
    CHECK_HIP(hipMalloc((void **)&df, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dff, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dg, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dgf, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dm, sizeof(float) * P));
    CHECK_HIP(hipMalloc((void **)&dmf, sizeof(float) * P));
    CHECK_HIP(hipMalloc((void **)&dq, sizeof(float) * NK * P));
    CHECK_HIP(hipMalloc((void **)&dqf, sizeof(float) * NK * P));
    CHECK_HIP(hipMalloc((void **)&dacc, accb));
    CHECK_HIP(hipMemcpy(df, hf, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dff, hff, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dg, hg, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dgf, hgf, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dm, hm, sizeof(float) * P, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dmf, hmf, sizeof(float) * P, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dq, hq, sizeof(float) * NK * P, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dqf, hqf, sizeof(float) * NK * P, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dacc, 0, accb));

    const int64_t sB = P, sT = (int64_t)X * Y, sX = Y;
    pre_field_t f = {df, sB, sT, sX, 1}, g = {dg, sB, sT, sX, 1};
    pre_screencells_t sc = {dq, NK, P, sT, sX, dm, sT, sX, 1, 1, 1, dacc, dacc + B, B};
    pre_field_t ff = {dff, sB, 1, (int64_t)Y * T, T}, gf = {dgf, sB, 1, (int64_t)Y * T, T};
    pre_screencellsflat_t scf = {dqf, NK, P, 1, (int64_t)Y * T, T, dmf, 1, (int64_t)Y * T, T, 1, 1, 1, dacc, dacc + B, B};

    /* the reference: interior cells, d = S(a) - S(b) in double from the fp32 inputs; with and without the modulation */
    double *want_s = calloc(2 * B, sizeof(double));
    unsigned *want_c = calloc(2 * NK * B, sizeof(unsigned)), *und = calloc(2 * NK * B, sizeof(unsigned));
    double rmax = 0.0, amax = 0.0, bmax = 0.0;
    for (int pass = 0; pass < 2; ++pass)
        for (int b = 0; b < B; ++b) for (int t = 1; t < T - 1; ++t) for (int x = 1; x < X - 1; ++x) for (int y = 1; y < Y - 1; ++y) {
            double half[2];
            for (int h = 0; h < 2; ++h) {
                const float *p = h ? hg : hf;
                half[h] = tw[0] * cell(p, b, t, x, y) + tw[1] * cell(p, b, t - 1, x, y) + tw[2] * cell(p, b, t + 1, x, y) +
                          tw[3] * cell(p, b, t, x - 1, y) + tw[4] * cell(p, b, t, x + 1, y) + tw[5] * cell(p, b, t, x, y - 1) +
                          tw[6] * cell(p, b, t, x, y + 1);
            }
            const double r = half[0] - half[1];
            if (pass == 0) { amax = fmax(amax, fabs(half[0])); bmax = fmax(bmax, fabs(half[1])); rmax = amax + bmax; continue; }
            for (int w = 0; w < 2; ++w) {                  /* w = 0: with the modulation, 1: without */
                const double m = w == 0 ? hm[pat(t, x, y)] : 1.0;
                want_s[w * B + b] = fmax(want_s[w * B + b], fabs(r) / m);
                for (int k = 0; k < NK; ++k) {
                    const double hw = (double)hq[(size_t)k * P + pat(t, x, y)] * m;
                    if (fabs(r) <= hw) ++want_c[(w * NK + k) * B + b];
                    if (fabs(fabs(r) - hw) <= 1e-5 * rmax) ++und[(w * NK + k) * B + b];
                }
            }
        }

    uint32_t *whole = malloc(accb), *other = malloc(accb);
    int rc = pre_screencellspair_stencil3d_f32(&f, &g, tw, toff, 7, &sc, B, T, X, Y, 0, NULL);
    EXPECT(rc == PRE_OK, "pre_screencellspair_stencil3d_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(whole, dacc, accb, hipMemcpyDeviceToHost));
    EXPECT(matches(whole, want_s, want_c, und, rmax), "Ny-fastest: scores and per-cell counts match the C loops, B = G + 1");

    CHECK_HIP(hipMemset(dacc, 0, accb));
    pre_screencells_t nomod = sc;
    nomod.modulation = NULL;
    rc = pre_screencellspair_stencil3d_f32(&f, &g, tw, toff, 7, &nomod, B, T, X, Y, 0, NULL);
    EXPECT(rc == PRE_OK, "without a modulation");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(other, dacc, accb, hipMemcpyDeviceToHost));
    EXPECT(matches(other, want_s + B, want_c + NK * B, und + NK * B, rmax), "without a modulation: hw is the level itself");

    CHECK_HIP(hipMemset(dacc, 0, accb));
    rc = pre_screencellspair_flat_stencil3d_f32(&ff, &gf, tw, toff, 7, &scf, B, T, X, Y, 0, NULL);
    EXPECT(rc == PRE_OK, "pre_screencellspair_flat_stencil3d_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(other, dacc, accb, hipMemcpyDeviceToHost));
    EXPECT(matches(other, want_s, want_c, und, rmax), "Nt-fastest: scores and per-cell counts match the C loops");

    /* the same grid as two t-slabs with their halo planes into fresh buffers */
    CHECK_HIP(hipMemset(dacc, 0, accb));
    pre_field_t f1 = {df + 2 * sT, sB, sT, sX, 1}, g1 = {dg + 2 * sT, sB, sT, sX, 1};
    pre_screencells_t s1 = sc;
    s1.modulation = dm + 2 * sT;
    s1.levels = dq + 2 * sT;
    rc = pre_screencellspair_stencil3d_f32(&f, &g, tw, toff, 7, &sc, B, 4, X, Y, 0, NULL);          /* planes 0..3: counts 1..2 */
    EXPECT(rc == PRE_OK, "first t-slab");
    rc = pre_screencellspair_stencil3d_f32(&f1, &g1, tw, toff, 7, &s1, B, 4, X, Y, 0, NULL);         /* planes 2..5: counts 3..4 */
    EXPECT(rc == PRE_OK, "second t-slab");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(other, dacc, accb, hipMemcpyDeviceToHost));
    EXPECT(memcmp(whole, other, accb) == 0, "two t-slabs accumulate to the bits of the whole grid");

    /* b == a: both halves round alike, every score is +0 and every cell with a non-negative band inside */
    CHECK_HIP(hipMemset(dacc, 0, accb));
    rc = pre_screencellspair_stencil3d_f32(&f, &f, tw, toff, 7, &sc, B, T, X, Y, 0, NULL);
    EXPECT(rc == PRE_OK, "b == a");
    rc = pre_screencellspair_flat_stencil3d_f32(&ff, &ff, tw, toff, 7, &scf, B, T, X, Y, 0, NULL);
    EXPECT(rc == PRE_OK, "flat: b == a");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(whole, dacc, accb, hipMemcpyDeviceToHost));
    {
        int zero = 1, all = 1;
        for (int b = 0; b < B; ++b) {
            if (whole[b] != 0u) zero = 0;
            for (int k = 0; k < NK; ++k) if (whole[(1 + k) * B + b] != 2u * (T - 2) * (X - 2) * (Y - 2)) all = 0;
        }
        EXPECT(zero, "b == a: every score has the bits of +0, in both forms");
        EXPECT(all, "b == a: every counted cell inside at every level, in both forms");
    }
    CHECK_HIP(hipMemcpy(dacc, other, accb, hipMemcpyHostToDevice));

    /* ---- argument errors: nothing is launched */
    EXPECT(pre_screencellspair_stencil3d_f32(&f, NULL, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null second set -> PRE_E_NULL");
    EXPECT(pre_screencellspair_stencil3d_f32(&f, &gf, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "second set Nt-fastest -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screencellspair_flat_stencil3d_f32(&ff, &g, tw, toff, 7, &scf, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "flat: second set Ny-fastest -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screencellspair_stencil3d_f32(NULL, &g, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null field -> PRE_E_NULL");
    EXPECT(pre_screencellspair_stencil3d_f32(&f, &g, tw, toff, 7, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null pre_screencells_t -> PRE_E_NULL");
    pre_screencells_t bad = sc;
    bad.levels = NULL;
    EXPECT(pre_screencellspair_stencil3d_f32(&f, &g, tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null levels -> PRE_E_NULL");
    bad = sc;
    bad.nk = 17;
    EXPECT(pre_screencellspair_stencil3d_f32(&f, &g, tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "17 levels -> PRE_E_RANGE");
    bad = sc;
    bad.lK = -1;
    EXPECT(pre_screencellspair_stencil3d_f32(&f, &g, tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_SHAPE, "negative level stride -> PRE_E_SHAPE");
    EXPECT(pre_screencellspair_stencil3d_f32(&ff, &gf, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "Nt-fastest view -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screencellspair_stencil3d_f32(&f, &g, tw, toff, 7, &sc, B, T, X, Y - 1, 0, NULL) == PRE_E_UNSUPPORTED, "width 67 -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screencellspair_flat_stencil3d_f32(&f, &g, tw, toff, 7, &scf, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "flat: Ny-fastest view -> PRE_E_UNSUPPORTED");
    pre_screencellsflat_t badf = scf;
    badf.lT = sT; badf.lX = sX; badf.lY = 1;
    EXPECT(pre_screencellspair_flat_stencil3d_f32(&ff, &gf, tw, toff, 7, &badf, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "flat: Ny-fastest levels -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screencellspair_flat_stencil3d_f32(&ff, &gf, tw, toff, 7, &scf, B, T, X, Y, PRE_FLAG_HALO_X, NULL) == PRE_E_UNSUPPORTED, "flat: PRE_FLAG_HALO_X -> PRE_E_UNSUPPORTED");
    float K[27] = {0}, Kbox[27] = {0};
    K[13] = 1.0f; Kbox[0] = 1.0f;
    pre_field_t three[3];
    for (int i = 0; i < 3; ++i) three[i] = f;
    EXPECT(pre_screencellspair_linear2_f32(three, three, K, NULL, 1.0f, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "linear2: null kernel");
    EXPECT(pre_screencellspair_linear2_f32(three, NULL, K, K, 1.0f, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "linear2: null second set");
    EXPECT(pre_screencellspair_ns_momentum_f32(three, three, K, Kbox, K, K, 0.1f, 0.1f, 0.1f, 0.1f, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED,
           "NS: kernel off the star -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screencellspair_mhd_continuity_f32(NULL, three, K, K, K, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "mhd continuity: null first set");
    EXPECT(pre_screencellspair_flat_ns_momentum_f32(three, three, K, K, K, K, 0.1f, 0.1f, 0.1f, 0.1f, &scf, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED,
           "flat NS: Ny-fastest sets -> PRE_E_UNSUPPORTED");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(whole, dacc, accb, hipMemcpyDeviceToHost));
    EXPECT(memcmp(whole, other, accb) == 0, "refused calls changed nothing");
    hipFree(df); hipFree(dff); hipFree(dg); hipFree(dgf); hipFree(dm); hipFree(dmf); hipFree(dq); hipFree(dqf); hipFree(dacc);
    free(hf); free(hff); free(hg); free(hgf); free(hm); free(hmf); free(hq); free(hqf); free(want_s); free(want_c); free(und); free(whole); free(other);
    return failures ? 1 : 0;
}
