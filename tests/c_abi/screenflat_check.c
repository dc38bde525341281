/* A C99 client of libcp_pre_screenflat.so: a tiny Nt-FASTEST batch (memory [B,X,Y,T]) screened with a 7-point star, the NS
 * momentum residual and the MHD continuity equation against three levels, checked against plain C loops (the definitions of
 * cp_pre_screenflat.h; Joint/NS_Residuals_CP.py:318-329), accumulation over two calls, PRE_FLAG_INTERIOR_T, plus the
 * PRE_E_UNSUPPORTED / PRE_E_RANGE / PRE_E_NULL cases of the header.  Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/screenflat_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_screenflat.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o screenflat_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_screenflat.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

/* T = 6 and Y = 10: rows of 6 cells, every other row end inside a quad */
enum { B = 2, T = 6, X = 5, Y = 10, CELLS = T * X * Y, NF = 6, NK = 3 };

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f - 0.5f; }
/* Nt-fastest: memory [B][X][Y][T] */
static size_t at(int b, int t, int x, int y) { return (((size_t)b * X + x) * Y + y) * T + t; }
static double cell(const float *f, int b, int t, int x, int y)
{
    return (t >= 0 && t < T && x >= 0 && x < X && y >= 0 && y < Y) ? (double)f[at(b, t, x, y)] : 0.0;
}
/* a dense 3x3x3 kernel on (T, X, Y) applied at one cell, zero padding */
static double op(const float *K, const float *f, int b, int t, int x, int y)
{
    double s = 0.0;
    for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) for (int d = 0; d < 3; ++d)
        if (K[(a * 3 + c) * 3 + d] != 0.0f) s += (double)K[(a * 3 + c) * 3 + d] * cell(f, b, t + a - 1, x + c - 1, y + d - 1);
    return s;
}

static float Kt[27], Kx[27], Ky[27], Kl[27], Ks[27];
static const float DT = 0.01f, DX = 0.02f, DY = 0.04f, NU = 0.003f;

/* residual `which` (0 star, 1 NS momentum, 2 MHD continuity) of the fields f[0..] at one cell, in double */
static double residual(int which, float *const *f, int b, int t, int x, int y)
{
    if (which == 0) return op(Ks, f[0], b, t, x, y);
    if (which == 1) {
        const float *u = f[0], *v = f[1], *p = f[2];
        const double uc = cell(u, b, t, x, y), vc = cell(v, b, t, x, y);
        const double dxdy = (double)(DX * DY), dtdy = (double)(DT * DY), dtdx = (double)(DT * DX), nudt = (double)(NU * DT);
        const double rx = op(Kt, u, b, t, x, y) * dxdy + uc * op(Kx, u, b, t, x, y) * dtdy + vc * op(Ky, u, b, t, x, y) * dtdx -
                          op(Kl, u, b, t, x, y) * nudt + op(Kx, p, b, t, x, y) * dtdy;
        const double ry = op(Kt, v, b, t, x, y) * dxdy + uc * op(Kx, v, b, t, x, y) * dtdx + vc * op(Ky, v, b, t, x, y) * dtdy -
                          op(Kl, v, b, t, x, y) * nudt + op(Ky, p, b, t, x, y) * dtdx;
        return rx + ry;
    }
    {
        const float *rho = f[0], *u = f[1], *v = f[2];
        const double rc = cell(rho, b, t, x, y);
        return op(Kt, rho, b, t, x, y) + cell(u, b, t, x, y) * op(Kx, rho, b, t, x, y) + rc * op(Kx, u, b, t, x, y) +
               cell(v, b, t, x, y) * op(Ky, rho, b, t, x, y) + rc * op(Ky, v, b, t, x, y);
    }
}

static const float hq[NK] = {0.5f, 1.5f, 1.0e6f};

/* compare the accumulators `acc` ([NK + 1][B]) with the loops over t in [1, T-1), x in [1, X-1), y in [1, Y-1) */
static int matches(int which, float *const *hf, const float *hm, const uint32_t *acc, const char *name)
{
    double rmax = 0.0;
    int ok = 1;
    for (int pass = 0; pass < 2 && ok; ++pass)
        for (int b = 0; b < B; ++b) {
            double want_s = 0.0;
            long want_c[NK] = {0, 0, 0}, und[NK] = {0, 0, 0};
            for (int t = 1; t < T - 1; ++t) for (int x = 1; x < X - 1; ++x) for (int y = 1; y < Y - 1; ++y) {
                const double r = fabs(residual(which, hf, b, t, x, y)), m = hm[((size_t)x * Y + y) * T + t];
                if (pass == 0) { rmax = fmax(rmax, r); continue; }
                want_s = fmax(want_s, r / m);
                for (int k = 0; k < NK; ++k) {
                    if (r <= (double)hq[k] * m) ++want_c[k];
                    if (fabs(r - (double)hq[k] * m) <= 1e-5 * rmax) ++und[k];
                }
            }
            if (pass == 0) continue;
            float got;
            memcpy(&got, &acc[b], sizeof(float));
            printf("      %s sample %d: score %.7g (C loop %.7g), counts %u %u %u (C loop %ld %ld %ld)\n", name, b, got, want_s,
                   acc[B + b], acc[2 * B + b], acc[3 * B + b], want_c[0], want_c[1], want_c[2]);
            if (!(fabs(got - want_s) <= 1e-5 * rmax / 0.75 + 1e-6 * want_s)) ok = 0;
            for (int k = 0; k < NK; ++k)
                if (labs((long)acc[(1 + k) * B + b] - want_c[k]) > und[k]) ok = 0;
            if (acc[3 * B + b] != (T - 2) * (X - 2) * (Y - 2)) ok = 0;      /* a level above every score holds every counted cell */
        }
    return ok;
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_screenflat_abi_version() == PRE_SCREENFLAT_ABI_VERSION, "pre_screenflat_abi_version");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    /* operators on (T, X, Y): index (a * 3 + c) * 3 + d = offset (a - 1, c - 1, d - 1) */
    Kt[(0 * 3 + 1) * 3 + 1] = -0.5f; Kt[(2 * 3 + 1) * 3 + 1] = 0.5f;
    Kx[(1 * 3 + 0) * 3 + 1] = -0.5f; Kx[(1 * 3 + 2) * 3 + 1] = 0.5f;
    Ky[(1 * 3 + 1) * 3 + 0] = -0.5f; Ky[(1 * 3 + 1) * 3 + 2] = 0.5f;
    Kl[13] = -4.0f; Kl[(1 * 3 + 0) * 3 + 1] = Kl[(1 * 3 + 2) * 3 + 1] = Kl[(1 * 3 + 1) * 3 + 0] = Kl[(1 * 3 + 1) * 3 + 2] = 1.0f;
    /* an asymmetric 7-point star as a tap list */
    const float tw[7] = {-1.75f, 0.5f, -1.25f, 0.875f, -0.375f, 1.5f, -0.625f};
    const int32_t toff[21] = {0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1};
    for (int i = 0; i < 7; ++i) Ks[((toff[3 * i] + 1) * 3 + toff[3 * i + 1] + 1) * 3 + toff[3 * i + 2] + 1] = tw[i];

    float *hf[NF], *hm = malloc(sizeof(float) * CELLS);
    unsigned s = 5u;
    for (int c = 0; c < NF; ++c) {
        hf[c] = malloc(sizeof(float) * B * CELLS);
        for (int i = 0; i < B * CELLS; ++i) hf[c][i] = 1.0f + 0.1f * (float)c + frand(&s);
    }
    for (int i = 0; i < CELLS; ++i) hm[i] = 0.75f + 0.5f * (frand(&s) + 0.5f);

    float *df, *dm, *dq;
    uint32_t *dacc;
    CHECK_HIP(hipMalloc((void **)&df, sizeof(float) * NF * B * CELLS));
    CHECK_HIP(hipMalloc((void **)&dm, sizeof(float) * CELLS));
    CHECK_HIP(hipMalloc((void **)&dq, sizeof(float) * NK));
    CHECK_HIP(hipMalloc((void **)&dacc, sizeof(uint32_t) * (NK + 1) * B));
    for (int c = 0; c < NF; ++c) CHECK_HIP(hipMemcpy(df + (size_t)c * B * CELLS, hf[c], sizeof(float) * B * CELLS, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dm, hm, sizeof(float) * CELLS, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dq, hq, sizeof(float) * NK, hipMemcpyHostToDevice));

    pre_field_t f[NF];
    for (int c = 0; c < NF; ++c) {
        const pre_field_t v = {df + (size_t)c * B * CELLS, (int64_t)CELLS, 1, (int64_t)Y * T, T};       /* sB, sT, sX, sY */
        f[c] = v;
    }
    const pre_screenflat_t sc = {dq, NK, dm, 1, (int64_t)Y * T, T, 1, 1, 1, dacc, dacc + B, B};
    uint32_t acc[(NK + 1) * B], again[(NK + 1) * B];
    int rc;

    /* ---- the three residuals against the loops */
    CHECK_HIP(hipMemset(dacc, 0, sizeof(acc)));
    rc = pre_screenflat_stencil3d_f32(&f[0], tw, toff, 7, &sc, B, T, X, Y, 0, NULL);
    EXPECT(rc == PRE_OK, "pre_screenflat_stencil3d_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(acc, dacc, sizeof(acc), hipMemcpyDeviceToHost));
    EXPECT(matches(0, hf, hm, acc, "star"), "star: scores and counts match the C loops (crop, modulation)");

    /* the same call again without zeroing: the counts double, the score stays */
    rc = pre_screenflat_stencil3d_f32(&f[0], tw, toff, 7, &sc, B, T, X, Y, 0, NULL);
    EXPECT(rc == PRE_OK, "second call into the same buffers");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(again, dacc, sizeof(again), hipMemcpyDeviceToHost));
    {
        int ok = memcmp(acc, again, sizeof(uint32_t) * B) == 0;
        for (int i = B; i < (NK + 1) * B; ++i) ok = ok && again[i] == 2 * acc[i];
        EXPECT(ok, "two calls: counts doubled, score kept");
    }
    /* PRE_FLAG_INTERIOR_T on the logical t axis: ct = 0 with the flag is ct = 1 without it */
    CHECK_HIP(hipMemset(dacc, 0, sizeof(acc)));
    pre_screenflat_t sf = sc;
    sf.ct = 0;
    rc = pre_screenflat_stencil3d_f32(&f[0], tw, toff, 7, &sf, B, T, X, Y, PRE_FLAG_INTERIOR_T, NULL);
    EXPECT(rc == PRE_OK, "PRE_FLAG_INTERIOR_T with ct = 0");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(again, dacc, sizeof(again), hipMemcpyDeviceToHost));
    EXPECT(memcmp(acc, again, sizeof(acc)) == 0, "PRE_FLAG_INTERIOR_T with ct = 0 gives the bits of ct = 1");

    CHECK_HIP(hipMemset(dacc, 0, sizeof(acc)));
    rc = pre_screenflat_ns_momentum_f32(&f[0], &f[1], &f[2], Kt, Kx, Ky, Kl, DT, DX, DY, NU, &sc, B, T, X, Y, 0, NULL);
    EXPECT(rc == PRE_OK, "pre_screenflat_ns_momentum_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(acc, dacc, sizeof(acc), hipMemcpyDeviceToHost));
    EXPECT(matches(1, hf, hm, acc, "NS momentum"), "NS momentum: scores and counts match the C loops");

    CHECK_HIP(hipMemset(dacc, 0, sizeof(acc)));
    rc = pre_screenflat_mhd_f32(0, f, Kt, Kx, Ky, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL);
    EXPECT(rc == PRE_OK, "pre_screenflat_mhd_f32 (continuity) returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(acc, dacc, sizeof(acc), hipMemcpyDeviceToHost));
    EXPECT(matches(2, hf, hm, acc, "MHD continuity"), "MHD continuity: scores and counts match the C loops");

    /* ---- the cases of the header that are refused before any launch */
    const pre_field_t yfast = {df, (int64_t)CELLS, (int64_t)X * Y, Y, 1};
    EXPECT(pre_screenflat_stencil3d_f32(&yfast, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "unit-stride last axis -> PRE_E_UNSUPPORTED");
    const pre_field_t pitched = {df, (int64_t)CELLS, 1, (int64_t)Y * T, T + 2};
    EXPECT(pre_screenflat_stencil3d_f32(&pitched, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "rows not dense (sY != T) -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenflat_stencil3d_f32(&f[0], tw, toff, 7, &sc, B, T, X, Y, PRE_FLAG_HALO_X, NULL) == PRE_E_UNSUPPORTED, "PRE_FLAG_HALO_X -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenflat_stencil3d_f32(&f[0], tw, toff, 7, &sc, B, T, X, Y, PRE_FLAG_ABS, NULL) == PRE_E_UNSUPPORTED, "PRE_FLAG_ABS -> PRE_E_UNSUPPORTED");
    const pre_field_t t96 = {df, (int64_t)CELLS, 1, 96, 96};
    EXPECT(pre_screenflat_stencil3d_f32(&t96, tw, toff, 7, &sc, 1, 96, 1, 1, 0, NULL) == PRE_E_UNSUPPORTED, "T = 96 -> PRE_E_UNSUPPORTED");
    const pre_field_t odd = {df, (int64_t)CELLS, 1, 7 * 5, 5};
    EXPECT(pre_screenflat_stencil3d_f32(&odd, tw, toff, 7, &sc, 1, 5, 2, 7, 0, NULL) == PRE_E_UNSUPPORTED, "Y * T = 35 -> PRE_E_UNSUPPORTED");
    const pre_field_t y1 = {df, (int64_t)CELLS, 1, 4, 4};
    EXPECT(pre_screenflat_stencil3d_f32(&y1, tw, toff, 7, &sc, 1, 4, 2, 1, 0, NULL) == PRE_E_UNSUPPORTED, "Y = 1 -> PRE_E_UNSUPPORTED");
    pre_screenflat_t bad = sc;
    bad.mT = (int64_t)X * Y; bad.mX = Y; bad.mY = 1;
    EXPECT(pre_screenflat_stencil3d_f32(&f[0], tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "modulation with unit stride on Y -> PRE_E_UNSUPPORTED");
    const int32_t box[3] = {1, 1, 0};
    EXPECT(pre_screenflat_stencil3d_f32(&f[0], tw, box, 1, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "tap off the star -> PRE_E_UNSUPPORTED");
    float Kbox[27] = {0};
    Kbox[0] = 1.0f;
    EXPECT(pre_screenflat_ns_momentum_f32(&f[0], &f[1], &f[2], Kt, Kbox, Ky, Kl, DT, DX, DY, NU, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED,
           "NS: kernel off the star -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenflat_linear2_f32(&f[0], &f[1], Kx, Kbox, 1.0f, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "linear2: kernel off the star -> PRE_E_UNSUPPORTED");
    /* D_t with a tap along x as well: the general-star tap structure, which is not built for the momentum equation */
    float Ktx[27];
    memcpy(Ktx, Kt, sizeof(Ktx));
    Ktx[(1 * 3 + 0) * 3 + 1] = 0.25f;
    EXPECT(pre_screenflat_mhd_f32(1, f, Ktx, Kx, Ky, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "mhd momentum, general star -> PRE_E_UNSUPPORTED");
    bad = sc; bad.nk = 17;
    EXPECT(pre_screenflat_stencil3d_f32(&f[0], tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "17 levels -> PRE_E_RANGE");
    bad = sc; bad.nk = 0;
    EXPECT(pre_screenflat_linear2_f32(&f[0], &f[1], Kx, Ky, 1.0f, &bad, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "0 levels -> PRE_E_RANGE");
    bad = sc; bad.cy = -1;
    EXPECT(pre_screenflat_ns_momentum_f32(&f[0], &f[1], &f[2], Kt, Kx, Ky, Kl, DT, DX, DY, NU, &bad, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "negative crop -> PRE_E_RANGE");
    EXPECT(pre_screenflat_mhd_f32(4, f, Kt, Kx, Ky, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "mhd: eq 4 -> PRE_E_RANGE");
    EXPECT(pre_screenflat_stencil3d_f32(NULL, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null field -> PRE_E_NULL");
    EXPECT(pre_screenflat_stencil3d_f32(&f[0], tw, toff, 7, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null pre_screenflat_t -> PRE_E_NULL");
    EXPECT(pre_screenflat_stencil3d_f32(&f[0], NULL, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null tap weights -> PRE_E_NULL");
    EXPECT(pre_screenflat_stencil3d_f32(&f[0], tw, toff, 7, &sc, B, T, 0, Y, 0, NULL) == PRE_E_NULL, "empty extent -> PRE_E_NULL");
    EXPECT(pre_screenflat_linear2_f32(&f[0], &f[1], Kx, NULL, 1.0f, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "linear2: null kernel -> PRE_E_NULL");
    EXPECT(pre_screenflat_mhd_f32(0, NULL, Kt, Kx, Ky, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "mhd: null fields -> PRE_E_NULL");
    bad = sc; bad.q = NULL;
    EXPECT(pre_screenflat_stencil3d_f32(&f[0], tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null levels -> PRE_E_NULL");
    bad = sc; bad.count_ld = B - 1;
    EXPECT(pre_screenflat_stencil3d_f32(&f[0], tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_NULL, "count_ld < B -> PRE_E_NULL");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(again, dacc, sizeof(again), hipMemcpyDeviceToHost));
    EXPECT(memcmp(acc, again, sizeof(acc)) == 0, "refused calls changed nothing");

    hipFree(df); hipFree(dm); hipFree(dq); hipFree(dacc);
    for (int c = 0; c < NF; ++c) free(hf[c]);
    free(hm);
    return failures ? 1 : 0;
}
