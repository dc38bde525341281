/* A C99 client of libcp_pre_screenstats.so: every entry once in each form - a 7-point star, Ka(f0) + ratio Kb(f1), the NS
 * momentum residual and the MHD continuity equation on a tiny [B,T,X,Y] batch Ny-fastest and Nt-fastest, a 5-point star and
 * the Burgers residual on a tiny [B,Nt,Nx] batch in both layouts - checked against plain C loops written here (the
 * definitions of cp_pre_screenstats.h), accumulation over two calls, PRE_FLAG_INTERIOR_T, a workspace full of NaN, the
 * workspace query, and the argument errors the entries return before any device work.  Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/screenstats_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_screenstats.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o screenstats_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_screenstats.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 2, T = 6, X = 5, Y = 12, CELLS = T * X * Y, NF = 6, RT = 12, RX = 24, RP = RT * RX };

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f - 0.5f; }

/* ---- the 2-D family: host fields are [B][T][X][Y]; the device holds them Ny-fastest and Nt-fastest ([B][X][Y][T]) */
static double cell(const float *f, int b, int t, int x, int y)
{
    return (t >= 0 && t < T && x >= 0 && x < X && y >= 0 && y < Y) ? (double)f[(((size_t)b * T + t) * X + x) * Y + y] : 0.0;
}
static double op(const float *K, const float *f, int b, int t, int x, int y)
{
    double s = 0.0;
    for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) for (int d = 0; d < 3; ++d)
        if (K[(a * 3 + c) * 3 + d] != 0.0f) s += (double)K[(a * 3 + c) * 3 + d] * cell(f, b, t + a - 1, x + c - 1, y + d - 1);
    return s;
}
static float Kt[27], Kx[27], Ky[27], Kl[27], Ks[27];
static const float DT = 0.01f, DX = 0.02f, DY = 0.04f, NU = 0.003f, RATIO = 0.75f;

/* residual `which` (0 star, 1 Kx(f0) + ratio Ky(f1), 2 NS momentum, 3 MHD continuity) at one cell, in double */
static double residual(int which, float *const *f, int b, int t, int x, int y)
{
    if (which == 0) return op(Ks, f[0], b, t, x, y);
    if (which == 1) return op(Kx, f[0], b, t, x, y) + (double)RATIO * op(Ky, f[1], b, t, x, y);
    if (which == 2) {
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

/* what one call leaves in the caller's buffers */
typedef struct { uint32_t mx[B]; double sums[3 * B]; } result_t;

static int fetch(result_t *r, const uint32_t *dmx, const double *dsums)
{
    if (hipDeviceSynchronize() != hipSuccess) return 0;
    return hipMemcpy(r->mx, dmx, sizeof r->mx, hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(r->sums, dsums, sizeof r->sums, hipMemcpyDeviceToHost) == hipSuccess;
}

/* `got` against the four statistics `want` ([4][B]: sum, sum |r|, sum r^2, max |r|) of `n` cells, rmax = max |r| anywhere */
static int close_to(const result_t *got, double want[4][B], int n, double rmax, const char *name)
{
    const double tau = 1e-5 * rmax;
    int ok = 1;
    for (int b = 0; b < B; ++b) {
        float mx;
        memcpy(&mx, &got->mx[b], sizeof mx);
        printf("      %s sample %d: sum %.10g (%.10g) sum|r| %.10g (%.10g) sum r^2 %.10g (%.10g) max %.7g (%.7g)\n", name, b,
               got->sums[b], want[0][b], got->sums[B + b], want[1][b], got->sums[2 * B + b], want[2][b], mx, want[3][b]);
        if (!(fabs(got->sums[b] - want[0][b]) <= n * tau)) ok = 0;
        if (!(fabs(got->sums[B + b] - want[1][b]) <= n * tau)) ok = 0;
        if (!(fabs(got->sums[2 * B + b] - want[2][b]) <= n * tau * (2 * rmax + tau))) ok = 0;
        if (!(fabs(mx - want[3][b]) <= tau + 1.2e-7 * want[3][b])) ok = 0;
    }
    return ok;
}

static void loops2d(int which, float *const *hf, int ct, double want[4][B], double *rmax)
{
    *rmax = 0.0;
    for (int b = 0; b < B; ++b) {
        want[0][b] = want[1][b] = want[2][b] = want[3][b] = 0.0;
        for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
            const double r = residual(which, hf, b, t, x, y);
            *rmax = fmax(*rmax, fabs(r));
            if (t < ct || t >= T - ct || x < 1 || x >= X - 1 || y < 1 || y >= Y - 1) continue;
            want[0][b] += r; want[1][b] += fabs(r); want[2][b] += r * r; want[3][b] = fmax(want[3][b], fabs(r));
        }
    }
}

/* ---- the 1-D family: host field [B][RT][RX] */
static double cell1(const float *f, int b, int t, int x)
{
    return (t >= 0 && t < RT && x >= 0 && x < RX) ? (double)f[((size_t)b * RT + t) * RX + x] : 0.0;
}
static double conv9(const float *K, const float *f, int b, int t, int x)
{
    double r = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) r += (double)K[a * 3 + c] * cell1(f, b, t + a - 1, x + c - 1);
    return r;
}
static const float KS9[9] = {0.f, 0.5f, 0.f, 0.875f, -1.75f, -0.375f, 0.f, -1.25f, 0.f};
static const float KT9[9] = {0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
static const float KX9[9] = {0.f, 0.f, 0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f};
static const float KXX9[9] = {0.f, 0.f, 0.f, 1.f, -2.f, 1.f, 0.f, 0.f, 0.f};
static const float DXc = 0.015625f, DTc = 0.01f, NUc = 0.002f, C3c = 1.28f;
static double residual1(int which, const float *f, int b, int t, int x)
{
    if (which == 0) return conv9(KS9, f, b, t, x);
    return (double)DXc * conv9(KT9, f, b, t, x) + (double)DTc * cell1(f, b, t, x) * conv9(KX9, f, b, t, x) -
           (double)NUc * conv9(KXX9, f, b, t, x) * (double)C3c;
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_screenstats_abi_version() == PRE_SCREENSTATS_ABI_VERSION, "pre_screenstats_abi_version");
    /* the workspace query runs without a device */
    const int64_t wl_ny = pre_screenstats_workspace_len(PRE_SCREENSTATS_FORM_NY, B, T, X, Y);
    const int64_t wl_flat = pre_screenstats_workspace_len(PRE_SCREENSTATS_FORM_FLAT, B, T, X, Y);
    const int64_t wl_rows = pre_screenstats_workspace_len(PRE_SCREENSTATS_FORM_ROWS, B, RT, RX, 1);
    EXPECT(wl_ny == 3 * B && wl_flat == 3 * B, "workspace query: one workgroup per sample on the tiny 2-D grid");
    EXPECT(wl_rows >= 3 * B && wl_rows <= 3 * B * 8, "workspace query: the 1-D plane");
    EXPECT(pre_screenstats_workspace_len(3, B, T, X, Y) == 0 && pre_screenstats_workspace_len(PRE_SCREENSTATS_FORM_NY, 0, T, X, Y) == 0,
           "workspace query: unknown form or empty extent -> 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    Kt[(0 * 3 + 1) * 3 + 1] = -0.5f; Kt[(2 * 3 + 1) * 3 + 1] = 0.5f;
    Kx[(1 * 3 + 0) * 3 + 1] = -0.5f; Kx[(1 * 3 + 2) * 3 + 1] = 0.5f;
    Ky[(1 * 3 + 1) * 3 + 0] = -0.5f; Ky[(1 * 3 + 1) * 3 + 2] = 0.5f;
    Kl[13] = -4.0f; Kl[(1 * 3 + 0) * 3 + 1] = Kl[(1 * 3 + 2) * 3 + 1] = Kl[(1 * 3 + 1) * 3 + 0] = Kl[(1 * 3 + 1) * 3 + 2] = 1.0f;
    const float tw[7] = {-1.75f, 0.5f, -1.25f, 0.875f, -0.375f, 1.5f, -0.625f};
    const int32_t toff[21] = {0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1};
    for (int i = 0; i < 7; ++i) Ks[((toff[3 * i] + 1) * 3 + toff[3 * i + 1] + 1) * 3 + toff[3 * i + 2] + 1] = tw[i];

    /* host fields [B][T][X][Y], and the same values with memory [B][X][Y][T] */
    float *hf[NF], *hp = malloc(sizeof(float) * B * CELLS);
    float *dny, *dfl;
    unsigned sd = 5u;
    CHECK_HIP(hipMalloc((void **)&dny, sizeof(float) * NF * B * CELLS));
    CHECK_HIP(hipMalloc((void **)&dfl, sizeof(float) * NF * B * CELLS));
    for (int c = 0; c < NF; ++c) {
        hf[c] = malloc(sizeof(float) * B * CELLS);
        for (int i = 0; i < B * CELLS; ++i) hf[c][i] = 1.0f + 0.1f * (float)c + frand(&sd);
        for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y)
            hp[(((size_t)b * X + x) * Y + y) * T + t] = hf[c][(((size_t)b * T + t) * X + x) * Y + y];
        CHECK_HIP(hipMemcpy(dny + (size_t)c * B * CELLS, hf[c], sizeof(float) * B * CELLS, hipMemcpyHostToDevice));
        CHECK_HIP(hipMemcpy(dfl + (size_t)c * B * CELLS, hp, sizeof(float) * B * CELLS, hipMemcpyHostToDevice));
    }
    pre_field_t fny[NF], ffl[NF];
    for (int c = 0; c < NF; ++c) {
        const pre_field_t a = {dny + (size_t)c * B * CELLS, (int64_t)CELLS, (int64_t)X * Y, Y, 1};       /* sB, sT, sX, sY */
        const pre_field_t f = {dfl + (size_t)c * B * CELLS, (int64_t)CELLS, 1, (int64_t)Y * T, T};
        fny[c] = a; ffl[c] = f;
    }
    uint32_t *dmx;
    double *dsums, *dws;
    const int64_t WS = 64;                       /* more than any query above */
    CHECK_HIP(hipMalloc((void **)&dmx, sizeof(uint32_t) * B));
    CHECK_HIP(hipMalloc((void **)&dsums, sizeof(double) * 3 * B));
    CHECK_HIP(hipMalloc((void **)&dws, sizeof(double) * WS));
    EXPECT(wl_ny <= WS && wl_flat <= WS && wl_rows <= WS, "the test's workspace holds every query");
    const pre_screenstats_t sc = {1, 1, 1, dmx, dsums, B, dws, WS};
    static const char *rname[4] = {"star", "linear2", "NS momentum", "MHD continuity"};
    result_t got, again;
    double want[4][B], rmax;
    char what[160];
    int rc = PRE_OK;
    const int NCNT = (T - 2) * (X - 2) * (Y - 2);

    for (int form = 0; form < 2; ++form) {
        const pre_field_t *f = form ? ffl : fny;
        for (int which = 0; which < 4; ++which) {
            CHECK_HIP(hipMemset(dmx, 0, sizeof(uint32_t) * B));
            CHECK_HIP(hipMemset(dsums, 0, sizeof(double) * 3 * B));
            CHECK_HIP(hipMemset(dws, 0xff, sizeof(double) * WS));             /* a workspace full of NaN */
            if (which == 0) rc = form ? pre_screenstats_flat_stencil3d_f32(&f[0], tw, toff, 7, &sc, B, T, X, Y, 0, NULL)
                                      : pre_screenstats_stencil3d_f32(&f[0], tw, toff, 7, &sc, B, T, X, Y, 0, NULL);
            if (which == 1) rc = form ? pre_screenstats_flat_linear2_f32(&f[0], &f[1], Kx, Ky, RATIO, &sc, B, T, X, Y, 0, NULL)
                                      : pre_screenstats_linear2_f32(&f[0], &f[1], Kx, Ky, RATIO, &sc, B, T, X, Y, 0, NULL);
            if (which == 2) rc = form ? pre_screenstats_flat_ns_momentum_f32(&f[0], &f[1], &f[2], Kt, Kx, Ky, Kl, DT, DX, DY, NU, &sc, B, T, X, Y, 0, NULL)
                                      : pre_screenstats_ns_momentum_f32(&f[0], &f[1], &f[2], Kt, Kx, Ky, Kl, DT, DX, DY, NU, &sc, B, T, X, Y, 0, NULL);
            if (which == 3) rc = form ? pre_screenstats_flat_mhd_f32(0, f, Kt, Kx, Ky, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL)
                                      : pre_screenstats_mhd_f32(0, f, Kt, Kx, Ky, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL);
            snprintf(what, sizeof what, "%s, %s: PRE_OK", rname[which], form ? "Nt-fastest" : "Ny-fastest");
            EXPECT(rc == PRE_OK, what);
            EXPECT(fetch(&got, dmx, dsums), "results fetched");
            loops2d(which, hf, 1, want, &rmax);
            snprintf(what, sizeof what, "%s, %s: the four statistics match the C loops (NaN workspace)", rname[which], form ? "Nt-fastest" : "Ny-fastest");
            EXPECT(close_to(&got, want, NCNT, rmax, rname[which]), what);
        }
        /* the last residual again without zeroing: the sums double exactly, the maximum stays */
        rc = form ? pre_screenstats_flat_mhd_f32(0, f, Kt, Kx, Ky, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL)
                  : pre_screenstats_mhd_f32(0, f, Kt, Kx, Ky, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL);
        EXPECT(rc == PRE_OK && fetch(&again, dmx, dsums), "second call into the same buffers");
        {
            int ok = memcmp(got.mx, again.mx, sizeof got.mx) == 0;
            for (int i = 0; i < 3 * B; ++i) ok = ok && again.sums[i] == 2.0 * got.sums[i];
            EXPECT(ok, "two calls: sums doubled to the bit, maximum kept");
        }
        /* PRE_FLAG_INTERIOR_T with ct = 0 gives the bytes of ct = 1 */
        CHECK_HIP(hipMemset(dmx, 0, sizeof(uint32_t) * B));
        CHECK_HIP(hipMemset(dsums, 0, sizeof(double) * 3 * B));
        pre_screenstats_t s0 = sc;
        s0.ct = 0;
        rc = form ? pre_screenstats_flat_mhd_f32(0, f, Kt, Kx, Ky, 5.0 / 3.0, &s0, B, T, X, Y, PRE_FLAG_INTERIOR_T, NULL)
                  : pre_screenstats_mhd_f32(0, f, Kt, Kx, Ky, 5.0 / 3.0, &s0, B, T, X, Y, PRE_FLAG_INTERIOR_T, NULL);
        EXPECT(rc == PRE_OK && fetch(&again, dmx, dsums), "PRE_FLAG_INTERIOR_T with ct = 0");
        EXPECT(memcmp(&got, &again, sizeof got) == 0, "PRE_FLAG_INTERIOR_T with ct = 0 gives the bytes of ct = 1");
    }

    /* ---- the 1-D family, both layouts */
    float *h1 = malloc(sizeof(float) * B * RP), *h1t = malloc(sizeof(float) * B * RP), *d1, *d1t;
    for (int i = 0; i < B * RP; ++i) h1[i] = 1.0f + frand(&sd);
    for (int b = 0; b < B; ++b) for (int t = 0; t < RT; ++t) for (int x = 0; x < RX; ++x) h1t[(size_t)b * RP + x * RT + t] = h1[(size_t)b * RP + t * RX + x];
    CHECK_HIP(hipMalloc((void **)&d1, sizeof(float) * B * RP));
    CHECK_HIP(hipMalloc((void **)&d1t, sizeof(float) * B * RP));
    CHECK_HIP(hipMemcpy(d1, h1, sizeof(float) * B * RP, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d1t, h1t, sizeof(float) * B * RP, hipMemcpyHostToDevice));
    const int64_t sx[3] = {RP, RX, 1}, stt[3] = {RP, 1, RT};
    const pre_screenstats_t s1 = {1, 1, 0, dmx, dsums, B, dws, WS};
    static const float tw5[5] = {-1.75f, 0.5f, -1.25f, 0.875f, -0.375f};
    static const int32_t toff5[10] = {0, 0, -1, 0, 1, 0, 0, -1, 0, 1};
    for (int which = 0; which < 2; ++which) {
        double r1max = 0.0;
        for (int b = 0; b < B; ++b) {
            want[0][b] = want[1][b] = want[2][b] = want[3][b] = 0.0;
            for (int t = 0; t < RT; ++t) for (int x = 0; x < RX; ++x) {
                const double r = residual1(which, h1, b, t, x);
                r1max = fmax(r1max, fabs(r));
                if (t < 1 || t >= RT - 1 || x < 1 || x >= RX - 1) continue;
                want[0][b] += r; want[1][b] += fabs(r); want[2][b] += r * r; want[3][b] = fmax(want[3][b], fabs(r));
            }
        }
        for (int layout = 0; layout < 2; ++layout) {
            const float *u = layout ? d1t : d1;
            const int64_t *st = layout ? stt : sx;
            CHECK_HIP(hipMemset(dmx, 0, sizeof(uint32_t) * B));
            CHECK_HIP(hipMemset(dsums, 0, sizeof(double) * 3 * B));
            CHECK_HIP(hipMemset(dws, 0xff, sizeof(double) * WS));
            rc = which == 0 ? pre_screenstats_rows_stencil2d_f32(u, st, tw5, toff5, 5, &s1, B, RT, RX, 0, NULL)
                            : pre_screenstats_rows_burgers_f32(u, st, KT9, KX9, KXX9, DXc, DTc, NUc, C3c, &s1, B, RT, RX, 0, NULL);
            snprintf(what, sizeof what, "1-D %s, %s: PRE_OK", which ? "Burgers" : "star", layout ? "Nt-fastest" : "Nx-fastest");
            EXPECT(rc == PRE_OK && fetch(&got, dmx, dsums), what);
            snprintf(what, sizeof what, "1-D %s, %s: the four statistics match the C loops (NaN workspace)", which ? "Burgers" : "star", layout ? "Nt-fastest" : "Nx-fastest");
            EXPECT(close_to(&got, want, (RT - 2) * (RX - 2), r1max, which ? "Burgers" : "star5"), what);
        }
    }

    /* ---- argument errors: nothing is launched; the buffers keep the last results */
    EXPECT(fetch(&got, dmx, dsums), "results before the refused calls");
    static const int32_t corner[6] = {0, 0, 0, 0, 1, 1};
    pre_screenstats_t bad;
    EXPECT(pre_screenstats_stencil3d_f32(NULL, tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null field -> PRE_E_NULL");
    EXPECT(pre_screenstats_stencil3d_f32(&fny[0], tw, toff, 7, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null descriptor -> PRE_E_NULL");
    EXPECT(pre_screenstats_flat_stencil3d_f32(&ffl[0], NULL, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null tap weights -> PRE_E_NULL");
    EXPECT(pre_screenstats_mhd_f32(0, NULL, Kt, Kx, Ky, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null field array -> PRE_E_NULL");
    EXPECT(pre_screenstats_linear2_f32(&fny[0], &fny[1], NULL, Ky, RATIO, &sc, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null kernel -> PRE_E_NULL");
    bad = sc; bad.max_abs = NULL;
    EXPECT(pre_screenstats_stencil3d_f32(&fny[0], tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null max_abs -> PRE_E_NULL");
    bad = sc; bad.sums = NULL;
    EXPECT(pre_screenstats_flat_ns_momentum_f32(&ffl[0], &ffl[1], &ffl[2], Kt, Kx, Ky, Kl, DT, DX, DY, NU, &bad, B, T, X, Y, 0, NULL) == PRE_E_NULL,
           "null sums -> PRE_E_NULL");
    bad = sc; bad.workspace = NULL;
    EXPECT(pre_screenstats_ns_momentum_f32(&fny[0], &fny[1], &fny[2], Kt, Kx, Ky, Kl, DT, DX, DY, NU, &bad, B, T, X, Y, 0, NULL) == PRE_E_NULL,
           "null workspace -> PRE_E_NULL");
    bad = sc; bad.workspace_len = wl_ny - 1;
    EXPECT(pre_screenstats_stencil3d_f32(&fny[0], tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_NULL, "short workspace, Ny-fastest -> PRE_E_NULL");
    bad = sc; bad.workspace_len = wl_flat - 1;
    EXPECT(pre_screenstats_flat_linear2_f32(&ffl[0], &ffl[1], Kx, Ky, RATIO, &bad, B, T, X, Y, 0, NULL) == PRE_E_NULL, "short workspace, Nt-fastest -> PRE_E_NULL");
    bad = s1; bad.workspace_len = wl_rows - 1;
    EXPECT(pre_screenstats_rows_burgers_f32(d1, sx, KT9, KX9, KXX9, DXc, DTc, NUc, C3c, &bad, B, RT, RX, 0, NULL) == PRE_E_NULL, "short workspace, 1-D -> PRE_E_NULL");
    bad = sc; bad.sum_ld = B - 1;
    EXPECT(pre_screenstats_stencil3d_f32(&fny[0], tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_NULL, "sum_ld < B -> PRE_E_NULL");
    EXPECT(pre_screenstats_stencil3d_f32(&fny[0], tw, toff, 7, &sc, B, 0, X, Y, 0, NULL) == PRE_E_NULL, "empty extent -> PRE_E_NULL");
    bad = sc; bad.cx = -1;
    EXPECT(pre_screenstats_stencil3d_f32(&fny[0], tw, toff, 7, &bad, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "negative crop -> PRE_E_RANGE");
    bad = sc; bad.ct = -1;
    EXPECT(pre_screenstats_flat_mhd_f32(0, ffl, Kt, Kx, Ky, 5.0 / 3.0, &bad, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "negative crop, Nt-fastest -> PRE_E_RANGE");
    bad = s1; bad.cy = 1;
    EXPECT(pre_screenstats_rows_stencil2d_f32(d1, sx, tw5, toff5, 5, &bad, B, RT, RX, 0, NULL) == PRE_E_RANGE, "1-D: cy = 1 -> PRE_E_RANGE");
    EXPECT(pre_screenstats_mhd_f32(4, fny, Kt, Kx, Ky, 5.0 / 3.0, &sc, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "eq = 4 -> PRE_E_RANGE");
    EXPECT(pre_screenstats_stencil3d_f32(&fny[0], tw, toff, 7, &sc, B, T, X, Y - 1, 0, NULL) == PRE_E_UNSUPPORTED, "Y % 4 != 0 -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenstats_flat_stencil3d_f32(&ffl[0], tw, toff, 7, &sc, B, T, X, Y - 1, 0, NULL) == PRE_E_UNSUPPORTED, "layout the flat form does not take -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenstats_rows_stencil2d_f32(d1, sx, tw5, toff5, 5, &s1, B, RT, RX - 1, 0, NULL) == PRE_E_UNSUPPORTED, "1-D: width 23 -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenstats_stencil3d_f32(&ffl[0], tw, toff, 7, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "Nt-fastest view into the Ny-fastest entry -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenstats_stencil3d_f32(&fny[0], tw, corner, 2, &sc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "tap off the star -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenstats_stencil3d_f32(&fny[0], tw, toff, 7, &sc, B, T, X, Y, PRE_FLAG_ABS, NULL) == PRE_E_UNSUPPORTED, "PRE_FLAG_ABS -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenstats_flat_stencil3d_f32(&ffl[0], tw, toff, 7, &sc, B, T, X, Y, PRE_FLAG_HALO_X, NULL) == PRE_E_UNSUPPORTED, "PRE_FLAG_HALO_X, Nt-fastest -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenstats_rows_burgers_f32(d1, sx, KT9, KX9, KXX9, DXc, DTc, NUc, C3c, &s1, B, RT, RX, PRE_FLAG_INTERIOR_T, NULL) == PRE_E_UNSUPPORTED,
           "1-D: any flag -> PRE_E_UNSUPPORTED");
    EXPECT(fetch(&again, dmx, dsums) && memcmp(&got, &again, sizeof got) == 0, "refused calls changed nothing");

    hipFree(dny); hipFree(dfl); hipFree(d1); hipFree(d1t); hipFree(dmx); hipFree(dsums); hipFree(dws);
    for (int c = 0; c < NF; ++c) free(hf[c]);
    free(hp); free(h1); free(h1t);
    return failures ? 1 : 0;
}
