/* A C99 client of libcp_pre_vjpjorek.so: the vector-Jacobian products of the two reduced-MHD (JOREK) residuals on a tiny
 * Nt-fastest grid (memory [B,F,X,Y,T]) whose quads straddle row ends, for the reference's tap structure (D_t, D_Z, D_ZZ
 * along Nt; D_R, D_RR along Nx) with unequal taps, checked against plain C loops on the logical axes (the formulas of
 * cp_pre_vjpjorek.h), plus the argument errors the entry returns before any device work.
 * Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/vjpjorek_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_vjpjorek.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o vjpjorek_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_vjpjorek.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 2, T = 10, X = 7, Y = 6, N = B * T * X * Y, NF = 3 };     /* T % 4 = 2: quads straddle row ends; Y*T = 60 */
enum { RHO, PHI, TT };

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f; }

static int inside(int t, int x, int y) { return t >= 0 && t < T && x >= 0 && x < X && y >= 0 && y < Y; }
static size_t at(int b, int t, int x, int y) { return (((size_t)b * X + x) * Y + y) * T + t; }      /* memory [B,X,Y,T] */
static double cell(const double *f, int b, int t, int x, int y) { return inside(t, x, y) ? f[at(b, t, x, y)] : 0.0; }

/* K: dense 3x3x3, index (a,b,c) -> offset (a-1,b-1,c-1).  sign +1: D(f)(x) = sum_k K_k f(x+k); -1: D^T(g)(x) = sum_k K_k g(x-k) */
static double Dop(const double *K, const double *f, int b, int t, int x, int y, int sign)
{
    double acc = 0.0;
    for (int a = 0; a < 3; ++a) for (int bb = 0; bb < 3; ++bb) for (int c = 0; c < 3; ++c) {
        const double w = K[(a * 3 + bb) * 3 + c];
        if (w != 0.0) acc += w * cell(f, b, t + sign * (a - 1), x + sign * (bb - 1), y + sign * (c - 1));
    }
    return acc;
}

/* a whole field: D(f) (sign +1) or D^T(f) (-1) */
static double *Dfield(const double *K, const double *f, int sign)
{
    double *r = malloc(sizeof(double) * N);
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y)
        r[at(b, t, x, y)] = Dop(K, f, b, t, x, y, sign);
    return r;
}

static double *prod(const double *a, const double *b)
{
    double *r = malloc(sizeof(double) * N);
    for (int i = 0; i < N; ++i) r[i] = a[i] * b[i];
    return r;
}

/* J(f; s) = D_R^T(h s D_Z f) - D_Z^T(h s D_R f) as a whole field (s == NULL: 1) */
static double *Jfield(const double *kR, const double *kZ, const double *h, const double *f, const double *s)
{
    double *dz = Dfield(kZ, f, 1), *dr = Dfield(kR, f, 1);
    double *hs = malloc(sizeof(double) * N);
    for (int i = 0; i < N; ++i) hs[i] = s ? h[i] * s[i] : h[i];
    double *a = prod(hs, dz), *b = prod(hs, dr);
    double *ra = Dfield(kR, a, -1), *zb = Dfield(kZ, b, -1);
    for (int i = 0; i < N; ++i) ra[i] -= zb[i];
    free(dz); free(dr); free(hs); free(a); free(b); free(zb);
    return ra;
}

static float *hg, *ho, hR[Y * T];
static double *f[NF], *gg, *Rr, *h;
static float *dfld, *dg, *dout, *dscale, *dR;
static const float up = 1000.0f, hs_ = 0.25f;

static int run(int eq, const float *Kt, const float *KR, const float *KZ, const float *KRR, const float *KZZ, const float coef[4])
{
    int failures = 0;
    const int64_t sB = (int64_t)X * Y * T, sX = (int64_t)Y * T, sY = T;
    const int nc = 2 + eq;
    double kt[27], kR[27], kZ[27], kRR[27], kZZ[27];
    for (int i = 0; i < 27; ++i) { kt[i] = Kt[i]; kR[i] = KR[i]; kZ[i] = KZ[i]; kRR[i] = KRR[i]; kZZ[i] = KZZ[i]; }
    const double a0 = coef[0], a1 = coef[1], a2 = coef[2], a3 = coef[3];
    pre_field_t fg = {dg, sB, 1, sX, sY}, fR = {dR, 0, 1, 0, sY};
    pre_field_t fs[NF];
    pre_out_t os[NF];
    for (int i = 0; i < NF; ++i) {                       /* fields: one [B,3,X,Y,T] buffer; gradients: another */
        pre_field_t v = {dfld + i * sB, NF * sB, 1, sX, sY};
        pre_out_t o = {dout + i * sB, NF * sB, 1, sX, sY};
        fs[i] = v; os[i] = o;
    }
    const double *rho = f[RHO], *phi = f[PHI], *tt = f[TT];
    double *want[NF] = {calloc(N, sizeof(double)), calloc(N, sizeof(double)), calloc(N, sizeof(double))};
    double *dZphi = Dfield(kZ, phi, 1), *dRphi = Dfield(kR, phi, 1);
    double *gr = prod(gg, rho), *gT = prod(gg, tt), *grT = prod(gr, tt), *gq = malloc(sizeof(double) * N);
    for (int i = 0; i < N; ++i) gq[i] = gg[i] / Rr[i];
    double *yt = malloc(sizeof(double) * N);
    {
        double *p = Dfield(kRR, gg, -1), *q = Dfield(kR, gq, -1), *r = Dfield(kZZ, gg, -1);
        for (int i = 0; i < N; ++i) yt[i] = p[i] + q[i] + r[i];
        free(p); free(q); free(r);
    }
    if (eq == 0) {
        double *dtg = Dfield(kt, gg, -1), *Jphi = Jfield(kR, kZ, h, phi, NULL), *Jrho = Jfield(kR, kZ, h, rho, NULL);
        double *zgr = Dfield(kZ, gr, -1);
        for (int i = 0; i < N; ++i) {
            want[RHO][i] = a0 * dtg[i] - a1 * Jphi[i] - a2 * gg[i] * dZphi[i] - a3 * yt[i];
            want[PHI][i] = a1 * Jrho[i] - a2 * zgr[i];
        }
        free(dtg); free(Jphi); free(Jrho); free(zgr);
    } else {
        double *dtgT = Dfield(kt, gT, -1), *dtgr = Dfield(kt, gr, -1), *dtT = Dfield(kt, tt, 1), *dtr = Dfield(kt, rho, 1);
        double *dRT = Dfield(kR, tt, 1), *dZT = Dfield(kZ, tt, 1), *dRr = Dfield(kR, rho, 1), *dZr = Dfield(kZ, rho, 1);
        double *JphiT = Jfield(kR, kZ, h, phi, tt), *Jphir = Jfield(kR, kZ, h, phi, rho);
        double *JTr = Jfield(kR, kZ, h, tt, rho), *JrT = Jfield(kR, kZ, h, rho, tt), *zgrT = Dfield(kZ, grT, -1);
        for (int i = 0; i < N; ++i) {
            const double XT = dRT[i] * dZphi[i] - dRphi[i] * dZT[i], Xr = dRr[i] * dZphi[i] - dRphi[i] * dZr[i];
            want[RHO][i] = dtgT[i] + gg[i] * dtT[i] - h[i] * XT + JphiT[i] + a0 * gg[i] * tt[i] * dZphi[i];
            want[TT][i] = gg[i] * dtr[i] + dtgr[i] - Jphir[i] + h[i] * Xr + a0 * gg[i] * rho[i] * dZphi[i] + a3 * yt[i];
            want[PHI][i] = JTr[i] - JrT[i] + a0 * zgrT[i];
        }
        free(dtgT); free(dtgr); free(dtT); free(dtr); free(dRT); free(dZT); free(dRr); free(dZr);
        free(JphiT); free(Jphir); free(JTr); free(JrT); free(zgrT);
    }
    CHECK_HIP(hipMemset(dout, 0xff, sizeof(float) * NF * N));
    const int rc = pre_vjpjorek_flat_f32(eq, &fg, fs, &fR, os, Kt, KR, KZ, KRR, KZZ, coef, hs_, dscale, B, T, X, Y, PRE_VJP_CROP, NULL);
    if (rc != PRE_OK) { printf("FAIL: eq %d returned %d\n", eq, rc); return failures + 1; }
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(ho, dout, sizeof(float) * NF * N, hipMemcpyDeviceToHost));
    int good = 1, untouched = 1;
    for (int c = 0; c < NF; ++c) {
        if (c >= nc) {                                   /* a slot the equation does not write keeps its fill */
            for (int b = 0; b < B; ++b) {
                const unsigned char *bytes = (const unsigned char *)(ho + ((size_t)b * NF + c) * sB);
                for (size_t j = 0; j < sizeof(float) * (size_t)sB; ++j) if (bytes[j] != 0xff) untouched = 0;
            }
            continue;
        }
        double err = 0, scale = 0;
        for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
            const double got = ho[(size_t)(b * NF + c) * sB + ((size_t)x * Y + y) * T + t], w = want[c][at(b, t, x, y)];
            err = fmax(err, fabs(got - w)); scale = fmax(scale, fabs(w));
        }
        printf("      eq %d field %d: max err %.3e of scale %.3e\n", eq, c, err, scale);
        if (!(err <= 1e-5 * scale) || !(scale > 0)) good = 0;
    }
    char what[160];
    snprintf(what, sizeof what, "equation %d: every gradient matches the C loops (crop, device scale, straddling quads, corners)", eq);
    EXPECT(good, what);
    snprintf(what, sizeof what, "equation %d: the slots of the fields it does not read are not written", eq);
    EXPECT(untouched, what);
    for (int c = 0; c < NF; ++c) free(want[c]);
    free(dZphi); free(dRphi); free(gr); free(gT); free(grT); free(gq); free(yt);
    return failures;
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_vjpjorek_abi_version() == PRE_VJPJOREK_ABI_VERSION, "pre_vjpjorek_abi_version");
    /* unequal taps on every axis an operator has any: a mirrored or swapped tap shows.  Index (t,x,y) -> (t*3 + x)*3 + y */
    float Kt[27] = {0}, KR[27] = {0}, KZ[27] = {0}, KRR[27] = {0}, KZZ[27] = {0}, KZy[27] = {0}, Kstar[27] = {0}, Kbox[27] = {0};
    Kt[4] = -1.0f; Kt[13] = 0.125f; Kt[22] = 1.5f;
    KR[10] = -0.75f; KR[16] = 1.25f;
    KZ[4] = -0.5f; KZ[22] = 0.875f;                      /* the reference's construction: D_Z along Nt */
    KRR[10] = 1.0f; KRR[13] = -2.25f; KRR[16] = 1.5f;
    KZZ[4] = 0.75f; KZZ[13] = -1.75f; KZZ[22] = 1.25f;
    KZy[12] = -0.5f; KZy[14] = 0.875f;                   /* D_Z along Ny (y_axis_fix) */
    Kstar[4] = 1.0f; Kstar[10] = 2.0f; Kstar[12] = 3.0f; /* a general star */
    Kbox[0] = 1.0f;
    const float cc[4] = {1.25f, 0.75f, 2.0f, 3.4f}, ct[4] = {10.0f / 3.0f, 0.0f, 0.0f, 0.75f};
    EXPECT(pre_vjpjorek_supported(0, Kt, KR, KZ, KRR, KZZ) == PRE_OK, "supported: the reference's tap structure, continuity");
    EXPECT(pre_vjpjorek_supported(1, Kt, KR, KZ, KRR, KZZ) == PRE_OK, "supported: the reference's tap structure, temperature");
    EXPECT(pre_vjpjorek_supported(0, Kt, KR, KZy, KRR, KZZ) == PRE_E_UNSUPPORTED, "supported: D_Z along Ny is not built");
    EXPECT(pre_vjpjorek_supported(1, Kt, Kstar, KZ, KRR, KZZ) == PRE_E_UNSUPPORTED, "supported: a general D_R is not built");
    EXPECT(pre_vjpjorek_supported(1, Kt, KR, KZ, KRR, KZy) == PRE_E_UNSUPPORTED, "supported: D_ZZ off D_Z's axis is not built");
    EXPECT(pre_vjpjorek_supported(0, Kt, Kbox, KZ, KRR, KZZ) == PRE_E_UNSUPPORTED, "supported: weight off the star");
    EXPECT(pre_vjpjorek_supported(2, Kt, KR, KZ, KRR, KZZ) == PRE_E_RANGE, "supported: eq out of range");
    EXPECT(pre_vjpjorek_supported(0, Kt, NULL, KZ, KRR, KZZ) == PRE_E_NULL, "supported: a null kernel");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    unsigned s = 17u;
    hg = malloc(sizeof(float) * N); ho = malloc(sizeof(float) * NF * N); gg = malloc(sizeof(double) * N);
    Rr = malloc(sizeof(double) * N); h = malloc(sizeof(double) * N);
    float *hall = malloc(sizeof(float) * NF * N), *hf[NF];
    for (int i = 0; i < NF; ++i) { hf[i] = malloc(sizeof(float) * N); f[i] = malloc(sizeof(double) * N); }
    for (int i = 0; i < N; ++i) {
        hg[i] = frand(&s) - 0.5f;
        for (int c = 0; c < NF; ++c) { hf[c][i] = 0.5f + frand(&s); f[c][i] = hf[c][i]; }
    }
    for (int b = 0; b < B; ++b) for (int c = 0; c < NF; ++c)
        memcpy(hall + ((size_t)b * NF + c) * (N / B), hf[c] + (size_t)b * (N / B), sizeof(float) * (N / B));
    for (int y = 0; y < Y; ++y) for (int t = 0; t < T; ++t) hR[y * T + t] = 1.0f + (float)y / (float)(Y - 1);      /* the row repeated */
    CHECK_HIP(hipMalloc((void **)&dg, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dfld, sizeof(float) * NF * N));
    CHECK_HIP(hipMalloc((void **)&dout, sizeof(float) * NF * N));
    CHECK_HIP(hipMalloc((void **)&dscale, sizeof(float)));
    CHECK_HIP(hipMalloc((void **)&dR, sizeof(float) * Y * T));
    CHECK_HIP(hipMemcpy(dg, hg, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dfld, hall, sizeof(float) * NF * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dscale, &up, sizeof(float), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dR, hR, sizeof(float) * Y * T, hipMemcpyHostToDevice));
    /* gg = hs * up * m * g with the crop mask, as the kernels form it on load; h = gg R */
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        const int m = t >= 1 && t <= T - 2 && x >= 1 && x <= X - 2 && y >= 1 && y <= Y - 2;
        const size_t i = at(b, t, x, y);
        gg[i] = m ? (double)hs_ * up * hg[i] : 0.0;
        Rr[i] = hR[y * T + t];
        h[i] = gg[i] * Rr[i];
    }
    int rc = run(0, Kt, KR, KZ, KRR, KZZ, cc);
    if (rc == 2) return 2;
    failures += rc;
    rc = run(1, Kt, KR, KZ, KRR, KZZ, ct);
    if (rc == 2) return 2;
    failures += rc;

    /* ---- argument errors: nothing is launched */
    const int64_t sB = (int64_t)X * Y * T, sX = (int64_t)Y * T, sY = T;
    pre_field_t fg = {dg, sB, 1, sX, sY}, fR = {dR, 0, 1, 0, sY};
    pre_field_t fs[NF];
    pre_out_t os[NF];
    for (int i = 0; i < NF; ++i) {
        pre_field_t v = {dfld + i * sB, NF * sB, 1, sX, sY};
        pre_out_t o = {dout + i * sB, NF * sB, 1, sX, sY};
        fs[i] = v; os[i] = o;
    }
#define CALL(eq, g, f_, r, o, kr, kz, t, y, flags) pre_vjpjorek_flat_f32(eq, g, f_, r, o, Kt, kr, kz, KRR, KZZ, ct, 1.0f, NULL, B, t, X, y, flags, NULL)
    EXPECT(CALL(1, NULL, fs, &fR, os, KR, KZ, T, Y, 0) == PRE_E_NULL, "null g -> PRE_E_NULL");
    EXPECT(CALL(1, &fg, NULL, &fR, os, KR, KZ, T, Y, 0) == PRE_E_NULL, "null fields -> PRE_E_NULL");
    EXPECT(CALL(1, &fg, fs, NULL, os, KR, KZ, T, Y, 0) == PRE_E_NULL, "null R -> PRE_E_NULL");
    EXPECT(CALL(1, &fg, fs, &fR, os, KR, KZ, 0, Y, 0) == PRE_E_NULL, "empty extent -> PRE_E_NULL");
    EXPECT(CALL(2, &fg, fs, &fR, os, KR, KZ, T, Y, 0) == PRE_E_RANGE, "eq out of range -> PRE_E_RANGE");
    EXPECT(CALL(0, &fg, fs, &fR, os, KR, KZy, T, Y, 0) == PRE_E_UNSUPPORTED, "D_Z along Ny -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(1, &fg, fs, &fR, os, Kstar, KZ, T, Y, 0) == PRE_E_UNSUPPORTED, "a general D_R -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(1, &fg, fs, &fR, os, Kbox, KZ, T, Y, 0) == PRE_E_UNSUPPORTED, "kernel off the star -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(1, &fg, fs, &fR, os, KR, KZ, T, Y, 2) == PRE_E_UNSUPPORTED, "a foreign flag -> PRE_E_UNSUPPORTED");
    pre_out_t alias[NF];
    memcpy(alias, os, sizeof os);
    alias[1].ptr = dfld + 2 * sB + 2;                    /* d phi over T */
    EXPECT(CALL(1, &fg, fs, &fR, alias, KR, KZ, T, Y, 0) == PRE_E_SHAPE, "d phi overlapping T -> PRE_E_SHAPE");
    memcpy(alias, os, sizeof os);
    alias[0].ptr = dR;
    EXPECT(CALL(1, &fg, fs, &fR, alias, KR, KZ, T, Y, 0) == PRE_E_SHAPE, "d rho over R -> PRE_E_SHAPE");
    pre_field_t yfast = {dg, (int64_t)T * X * Y, (int64_t)X * Y, Y, 1};
    EXPECT(CALL(1, &yfast, fs, &fR, os, KR, KZ, T, Y, 0) == PRE_E_UNSUPPORTED, "Ny-fastest g -> PRE_E_UNSUPPORTED");
    pre_field_t pitched[NF];
    memcpy(pitched, fs, sizeof fs);
    pitched[2].sY = sY + 2;
    EXPECT(CALL(1, &fg, pitched, &fR, os, KR, KZ, T, Y, 0) == PRE_E_UNSUPPORTED, "rows of T not dense -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(0, &fg, pitched, &fR, os, KR, KZ, T, Y, 0) == PRE_OK, "continuity ignores fields[2]");
    CHECK_HIP(hipDeviceSynchronize());
    pre_field_t Rbad = {dR, 0, 1, 0, sY + 1};
    EXPECT(CALL(1, &fg, fs, &Rbad, os, KR, KZ, T, Y, 0) == PRE_E_UNSUPPORTED, "R's rows not T apart -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(1, &fg, fs, &fR, os, KR, KZ, 96, Y, 0) == PRE_E_UNSUPPORTED, "T = 96 -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(1, &fg, fs, &fR, os, KR, KZ, 7, 9, 0) == PRE_E_UNSUPPORTED, "Y*T % 4 != 0 -> PRE_E_UNSUPPORTED");
#undef CALL
    hipFree(dg); hipFree(dfld); hipFree(dout); hipFree(dscale); hipFree(dR);
    for (int i = 0; i < NF; ++i) { free(hf[i]); free(f[i]); }
    free(hg); free(ho); free(gg); free(hall); free(Rr); free(h);
    return failures ? 1 : 0;
}
