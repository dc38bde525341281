/* A C99 client of libcp_pre_vjpflatmhd.so: the vector-Jacobian products of the four ideal-MHD residuals on a tiny Nt-fastest
 * grid (memory [B,F,X,Y,T]) whose quads straddle row ends, for the reference's tap structure (D_y along Nt) and for D_y
 * along Ny, checked against plain C loops on the logical axes (the formulas of cp_pre_vjpmhd.h), plus the argument errors
 * the entries return before any device work.
 * Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/vjpflatmhd_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_vjpflatmhd.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o vjpflatmhd_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_vjpflatmhd.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 2, T = 10, X = 7, Y = 6, N = B * T * X * Y, NF = 6 };     /* T % 4 = 2: quads straddle row ends; Y*T = 60 */
enum { RHO, U, V, P_, BX, BY };

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

static double *prod(const double *a, const double *b)
{
    double *r = malloc(sizeof(double) * N);
    for (int i = 0; i < N; ++i) r[i] = a[i] * b[i];
    return r;
}

static float *hf[NF], *hg, *ho;
static double *f[NF], *gg;
static float *dfld, *dg, *dout, *dscale;
static const float up = 1000.0f, hs = 0.25f;
static const double gamma_ = 5.0 / 3.0;

/* all four entries for one operator set; want[eq][field] by the header's formulas */
static int run(const float *Kt, const float *Kx, const float *Ky, const char *label)
{
    int failures = 0;
    const int64_t sB = (int64_t)X * Y * T, sX = (int64_t)Y * T, sY = T;
    double kt[27], kx[27], ky[27], km[27], kp[27];
    for (int i = 0; i < 27; ++i) { kt[i] = Kt[i]; kx[i] = Kx[i]; ky[i] = Ky[i]; km[i] = kx[i] - ky[i]; kp[i] = kx[i] + ky[i]; }
    pre_field_t fg = {dg, sB, 1, sX, sY};
    pre_field_t all[NF];
    pre_out_t oall[NF];
    for (int i = 0; i < NF; ++i) {                       /* fields: one [B,6,X,Y,T] buffer; gradients: another */
        pre_field_t v = {dfld + i * sB, NF * sB, 1, sX, sY};
        pre_out_t o = {dout + i * sB, NF * sB, 1, sX, sY};
        all[i] = v; oall[i] = o;
    }
    const double *rho = f[RHO], *u = f[U], *v = f[V], *p = f[P_], *bx = f[BX], *by = f[BY];
    double *gu = prod(gg, u), *gv = prod(gg, v), *gr = prod(gg, rho), *gbx = prod(gg, bx), *gby = prod(gg, by);
    double *q = malloc(sizeof(double) * N), *upv = malloc(sizeof(double) * N), *A = malloc(sizeof(double) * N);
    double *C = malloc(sizeof(double) * N), *W = malloc(sizeof(double) * N);
    for (int i = 0; i < N; ++i) {
        const double pg = p[i] - 0.5 * (bx[i] * bx[i] + by[i] * by[i]);
        q[i] = 1.0 / rho[i]; upv[i] = u[i] + v[i];
        A[i] = gamma_ * pg + by[i] * by[i]; C[i] = gamma_ * pg + bx[i] * bx[i]; W[i] = u[i] * bx[i] + v[i] * by[i];
    }
    double *gq = prod(gg, q), *gqbx = prod(gq, bx), *gqby = prod(gq, by), *gA = prod(gg, A), *gC = prod(gg, C);
    double *gE = prod(gbx, by), *gW = prod(gg, W);
    const double k = gamma_ - 2.0;

    for (int eq = 0; eq < 4; ++eq) {
        int rc;
        int chan[NF], nc;
        CHECK_HIP(hipMemset(dout, 0xff, sizeof(float) * NF * N));
        if (eq == PRE_VJPMHD_EQ_CONTINUITY) {
            const int c[3] = {RHO, U, V}; nc = 3; memcpy(chan, c, sizeof c);
        } else if (eq == PRE_VJPMHD_EQ_INDUCTION) {
            const int c[4] = {U, V, BX, BY}; nc = 4; memcpy(chan, c, sizeof c);
        } else {
            const int c[6] = {RHO, U, V, P_, BX, BY}; nc = 6; memcpy(chan, c, sizeof c);
        }
        pre_field_t fs[NF];
        pre_out_t os[NF];
        for (int i = 0; i < nc; ++i) { fs[i] = all[chan[i]]; os[i] = oall[chan[i]]; }
        if (eq == PRE_VJPMHD_EQ_CONTINUITY)
            rc = pre_vjpflatmhd_continuity_f32(&fg, fs, os, Kt, Kx, Ky, hs, dscale, B, T, X, Y, PRE_VJP_CROP, NULL);
        else if (eq == PRE_VJPMHD_EQ_INDUCTION)
            rc = pre_vjpflatmhd_induction_f32(&fg, fs, os, Kt, Kx, Ky, hs, dscale, B, T, X, Y, PRE_VJP_CROP, NULL);
        else if (eq == PRE_VJPMHD_EQ_MOMENTUM)
            rc = pre_vjpflatmhd_momentum_f32(&fg, fs, os, Kt, Kx, Ky, hs, dscale, B, T, X, Y, PRE_VJP_CROP, NULL);
        else
            rc = pre_vjpflatmhd_energy_f32(&fg, fs, os, Kt, Kx, Ky, gamma_, hs, dscale, B, T, X, Y, PRE_VJP_CROP, NULL);
        if (rc != PRE_OK) { printf("FAIL: %s eq %d returned %d\n", label, eq, rc); return failures + 1; }
        CHECK_HIP(hipDeviceSynchronize());
        CHECK_HIP(hipMemcpy(ho, dout, sizeof(float) * NF * N, hipMemcpyDeviceToHost));
        double err[NF] = {0}, scale[NF] = {0};
        for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
            const size_t i = at(b, t, x, y);
            const double g0 = gg[i];
            double want[NF] = {0};
#define D_(K, F) Dop(K, F, b, t, x, y, 1)
#define DT_(K, F) Dop(K, F, b, t, x, y, -1)
            if (eq == PRE_VJPMHD_EQ_CONTINUITY) {
                want[RHO] = DT_(kt, gg) + DT_(kx, gu) + DT_(ky, gv) + g0 * (D_(kx, u) + D_(ky, v));
                want[U] = g0 * D_(kx, rho) + DT_(kx, gr);
                want[V] = g0 * D_(ky, rho) + DT_(ky, gr);
            } else if (eq == PRE_VJPMHD_EQ_INDUCTION) {
                want[U] = DT_(km, gby) + g0 * D_(kp, by);
                want[V] = -DT_(km, gbx) - g0 * D_(kp, bx);
                want[BX] = DT_(kt, gg) - g0 * D_(km, v) - DT_(kp, gv);
                want[BY] = DT_(kt, gg) + g0 * D_(km, u) + DT_(kp, gu);
            } else if (eq == PRE_VJPMHD_EQ_MOMENTUM) {
                const double sx = 2 * D_(kx, bx) + D_(kp, by), sy = 2 * D_(ky, by) + D_(kp, bx);
                const double S = bx[i] * sx + by[i] * sy, TT = DT_(kt, gg) + DT_(kx, gu) + DT_(ky, gv);
                want[U] = TT + g0 * D_(kx, upv);
                want[V] = TT + g0 * D_(ky, upv);
                want[RHO] = -g0 * q[i] * q[i] * (D_(kp, p) - S);
                want[P_] = DT_(kp, gq);
                want[BX] = -(gq[i] * sx + 2 * DT_(kx, gqbx) + DT_(kp, gqby));
                want[BY] = -(gq[i] * sy + 2 * DT_(ky, gqby) + DT_(kp, gqbx));
            } else {
                const double dv = D_(kx, bx) + D_(ky, by), sh = D_(ky, u) + D_(kx, v);
                const double dxu = D_(kx, u), dyv = D_(ky, v);
                want[RHO] = DT_(kt, gg);
                want[U] = g0 * (D_(kx, p) + k * bx[i] * dv) + DT_(kx, gA) - DT_(ky, gE);
                want[V] = g0 * (D_(ky, p) + k * by[i] * dv) + DT_(ky, gC) - DT_(kx, gE);
                want[P_] = DT_(kx, gu) + DT_(ky, gv) + gamma_ * g0 * (dxu + dyv);
                want[BX] = k * (g0 * u[i] * dv + DT_(kx, gW)) + g0 * (bx[i] * ((2 - gamma_) * dyv - gamma_ * dxu) - by[i] * sh);
                want[BY] = k * (g0 * v[i] * dv + DT_(ky, gW)) + g0 * (by[i] * ((2 - gamma_) * dxu - gamma_ * dyv) - bx[i] * sh);
            }
#undef D_
#undef DT_
            for (int c = 0; c < nc; ++c) {
                const int ch = chan[c];
                const double got = ho[(size_t)(b * NF + ch) * sB + ((size_t)x * Y + y) * T + t];
                err[ch] = fmax(err[ch], fabs(got - want[ch]));
                scale[ch] = fmax(scale[ch], fabs(want[ch]));
            }
        }
        int good = 1, untouched = 1;
        for (int c = 0; c < nc; ++c) {
            printf("      %s eq %d field %d: max err %.3e of scale %.3e\n", label, eq, chan[c], err[chan[c]], scale[chan[c]]);
            if (!(err[chan[c]] <= 1e-5 * scale[chan[c]])) good = 0;
        }
        for (int ch = 0; ch < NF; ++ch) {                /* a slot the equation does not write keeps its fill */
            int mine = 0;
            for (int c = 0; c < nc; ++c) mine |= chan[c] == ch;
            if (mine) continue;
            for (int b = 0; b < B; ++b) {
                const unsigned char *bytes = (const unsigned char *)(ho + ((size_t)b * NF + ch) * sB);
                for (size_t j = 0; j < sizeof(float) * (size_t)sB; ++j) if (bytes[j] != 0xff) untouched = 0;
            }
        }
        char what[160];
        snprintf(what, sizeof what, "%s, equation %d: every gradient matches the C loops (crop, device scale, straddling quads)", label, eq);
        EXPECT(good, what);
        snprintf(what, sizeof what, "%s, equation %d: the slots of the fields it does not read are not written", label, eq);
        EXPECT(untouched, what);
    }
    free(gu); free(gv); free(gr); free(gbx); free(gby); free(q); free(upv); free(A); free(C); free(W);
    free(gq); free(gqbx); free(gqby); free(gA); free(gC); free(gE); free(gW);
    return failures;
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_vjpflatmhd_abi_version() == PRE_VJPFLATMHD_ABI_VERSION, "pre_vjpflatmhd_abi_version");
    /* unequal taps on every axis: a mirrored or swapped tap shows */
    float Kt[27] = {0}, Kx[27] = {0}, KyT[27] = {0}, KyY[27] = {0}, Kstar[27] = {0}, Kbox[27] = {0};
    Kt[4] = -1.0f; Kt[22] = 1.5f;
    Kx[10] = -0.75f; Kx[16] = 1.25f;
    KyT[4] = -0.5f; KyT[22] = 0.875f;                    /* the reference's construction: D_y along Nt */
    KyY[12] = -0.5f; KyY[14] = 0.875f;                   /* D_y along Ny */
    Kstar[4] = 1.0f; Kstar[10] = 2.0f; Kstar[12] = 3.0f; /* a general star */
    Kbox[0] = 1.0f;
    EXPECT(pre_vjpflatmhd_supported(PRE_VJPMHD_EQ_ENERGY, Kt, Kx, KyT) == PRE_OK, "supported: the reference's tap structure");
    EXPECT(pre_vjpflatmhd_supported(PRE_VJPMHD_EQ_ENERGY, Kt, Kx, KyY) == PRE_OK, "supported: D_y along Ny");
    EXPECT(pre_vjpflatmhd_supported(PRE_VJPMHD_EQ_ENERGY, Kt, Kstar, KyY) == PRE_E_UNSUPPORTED, "supported: energy with general stars is not built");
    EXPECT(pre_vjpflatmhd_supported(PRE_VJPMHD_EQ_MOMENTUM, Kt, Kstar, KyY) == PRE_E_UNSUPPORTED, "supported: momentum with general stars is not built");
    EXPECT(pre_vjpflatmhd_supported(PRE_VJPMHD_EQ_CONTINUITY, Kt, Kstar, KyY) == PRE_OK, "supported: continuity with general stars is built");
    EXPECT(pre_vjpflatmhd_supported(PRE_VJPMHD_EQ_INDUCTION, Kt, Kstar, KyY) == PRE_OK, "supported: induction with general stars is built");
    EXPECT(pre_vjpflatmhd_supported(PRE_VJPMHD_EQ_MOMENTUM, Kt, Kbox, KyY) == PRE_E_UNSUPPORTED, "supported: weight off the star");
    EXPECT(pre_vjpflatmhd_supported(7, Kt, Kx, KyY) == PRE_E_RANGE, "supported: eq out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    unsigned s = 17u;
    hg = malloc(sizeof(float) * N); ho = malloc(sizeof(float) * NF * N); gg = malloc(sizeof(double) * N);
    float *hall = malloc(sizeof(float) * NF * N);
    for (int i = 0; i < NF; ++i) { hf[i] = malloc(sizeof(float) * N); f[i] = malloc(sizeof(double) * N); }
    for (int i = 0; i < N; ++i) {
        hg[i] = frand(&s) - 0.5f;
        for (int c = 0; c < NF; ++c) { hf[c][i] = 0.5f + frand(&s); f[c][i] = hf[c][i]; }
    }
    for (int b = 0; b < B; ++b) for (int c = 0; c < NF; ++c)
        memcpy(hall + ((size_t)b * NF + c) * (N / B), hf[c] + (size_t)b * (N / B), sizeof(float) * (N / B));
    CHECK_HIP(hipMalloc((void **)&dg, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dfld, sizeof(float) * NF * N));
    CHECK_HIP(hipMalloc((void **)&dout, sizeof(float) * NF * N));
    CHECK_HIP(hipMalloc((void **)&dscale, sizeof(float)));
    CHECK_HIP(hipMemcpy(dg, hg, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dfld, hall, sizeof(float) * NF * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dscale, &up, sizeof(float), hipMemcpyHostToDevice));
    /* gg = hs * up * m * g with the crop mask, as the kernels form it on load */
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        const int m = t >= 1 && t <= T - 2 && x >= 1 && x <= X - 2 && y >= 1 && y <= Y - 2;
        gg[at(b, t, x, y)] = m ? (double)hs * up * hg[at(b, t, x, y)] : 0.0;
    }
    int rc = run(Kt, Kx, KyT, "D_y along Nt");
    if (rc == 2) return 2;
    failures += rc;
    rc = run(Kt, Kx, KyY, "D_y along Ny");
    if (rc == 2) return 2;
    failures += rc;

    /* ---- argument errors: nothing is launched */
    const int64_t sB = (int64_t)X * Y * T, sX = (int64_t)Y * T, sY = T;
    pre_field_t fg = {dg, sB, 1, sX, sY};
    pre_field_t fs[NF];
    pre_out_t os[NF];
    for (int i = 0; i < NF; ++i) {
        pre_field_t v = {dfld + i * sB, NF * sB, 1, sX, sY};
        pre_out_t o = {dout + i * sB, NF * sB, 1, sX, sY};
        fs[i] = v; os[i] = o;
    }
    EXPECT(pre_vjpflatmhd_momentum_f32(NULL, fs, os, Kt, Kx, KyY, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null g -> PRE_E_NULL");
    EXPECT(pre_vjpflatmhd_momentum_f32(&fg, NULL, os, Kt, Kx, KyY, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null fields -> PRE_E_NULL");
    EXPECT(pre_vjpflatmhd_energy_f32(&fg, fs, os, Kt, Kx, KyY, gamma_, 1.0f, NULL, B, 0, X, Y, 0, NULL) == PRE_E_NULL, "empty extent -> PRE_E_NULL");
    EXPECT(pre_vjpflatmhd_energy_f32(&fg, fs, os, Kt, Kstar, KyY, gamma_, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "energy, general stars -> PRE_E_UNSUPPORTED");
    EXPECT(pre_vjpflatmhd_continuity_f32(&fg, fs, os, Kt, Kbox, KyY, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "kernel off the star -> PRE_E_UNSUPPORTED");
    pre_out_t alias[NF];
    memcpy(alias, os, sizeof os);
    alias[1].ptr = dfld + 3 * sB + 2;                    /* du over p: written by launch A, read by launch B */
    EXPECT(pre_vjpflatmhd_momentum_f32(&fg, fs, alias, Kt, Kx, KyY, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_SHAPE, "momentum: du overlapping p -> PRE_E_SHAPE");
    pre_field_t yfast = {dg, (int64_t)T * X * Y, (int64_t)X * Y, Y, 1};
    EXPECT(pre_vjpflatmhd_induction_f32(&yfast, fs, os, Kt, Kx, KyY, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "Ny-fastest g -> PRE_E_UNSUPPORTED");
    pre_field_t pitched[NF];
    memcpy(pitched, fs, sizeof fs);
    pitched[5].sY = sY + 2;                              /* By: read by launch B only */
    EXPECT(pre_vjpflatmhd_momentum_f32(&fg, pitched, os, Kt, Kx, KyY, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "rows of a field not dense -> PRE_E_UNSUPPORTED");
    EXPECT(pre_vjpflatmhd_continuity_f32(&fg, fs, os, Kt, Kx, KyY, 1.0f, NULL, B, 96, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "T = 96 -> PRE_E_UNSUPPORTED");
    EXPECT(pre_vjpflatmhd_continuity_f32(&fg, fs, os, Kt, Kx, KyY, 1.0f, NULL, B, 7, X, 9, 0, NULL) == PRE_E_UNSUPPORTED, "Y*T % 4 != 0 -> PRE_E_UNSUPPORTED");
    EXPECT(pre_vjpflatmhd_momentum_f32(&fg, fs, os, Kt, Kstar, KyY, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "momentum, general stars -> PRE_E_UNSUPPORTED");
    hipFree(dg); hipFree(dfld); hipFree(dout); hipFree(dscale);
    for (int i = 0; i < NF; ++i) { free(hf[i]); free(f[i]); }
    free(hg); free(ho); free(gg); free(hall);
    return failures ? 1 : 0;
}
