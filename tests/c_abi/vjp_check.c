/* A C99 client of libcp_pre_vjp.so: the vector-Jacobian product of the wave star and of the NS momentum residual on a
 * tiny grid, and the deterministic sum of squares, checked against plain C loops (the formulas of cp_pre_vjp.h;
 * Physics_Informed/Wave_FNO_PISL.py:209-217), plus the argument errors the entries return before any device work.
 * Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/vjp_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_vjp.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o vjp_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_vjp.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 2, T = 5, X = 9, Y = 67, N = B * T * X * Y };     /* odd width: full quads and the partial last one */

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f - 0.5f; }

static int inside(int t, int x, int y) { return t >= 0 && t < T && x >= 0 && x < X && y >= 0 && y < Y; }
static size_t at(int b, int t, int x, int y) { return (((size_t)b * T + t) * X + x) * Y + y; }
static double cell(const double *f, int b, int t, int x, int y) { return inside(t, x, y) ? f[at(b, t, x, y)] : 0.0; }

/* K: dense 3x3x3, index (a,b,c) -> offset (a-1,b-1,c-1).  D(f)(x) = sum_k K_k f(x+k); DT(g)(x) = sum_k K_k g(x-k) */
static double Dop(const float *K, const double *f, int b, int t, int x, int y, int sign)
{
    double acc = 0.0;
    for (int a = 0; a < 3; ++a) for (int bb = 0; bb < 3; ++bb) for (int c = 0; c < 3; ++c) {
        const float w = K[(a * 3 + bb) * 3 + c];
        if (w != 0.0f) acc += (double)w * cell(f, b, t + sign * (a - 1), x + sign * (bb - 1), y + sign * (c - 1));
    }
    return acc;
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_vjp_abi_version() == PRE_VJP_ABI_VERSION, "pre_vjp_abi_version");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    float *hg = malloc(sizeof(float) * N), *hu = malloc(sizeof(float) * N), *hv = malloc(sizeof(float) * N);
    float *ho = malloc(sizeof(float) * 3 * N);
    double *gg = malloc(sizeof(double) * N), *gu = malloc(sizeof(double) * N), *gv = malloc(sizeof(double) * N);
    double *du_ = malloc(sizeof(double) * N), *dv_ = malloc(sizeof(double) * N);
    unsigned s = 11u;
    for (int i = 0; i < N; ++i) { hg[i] = frand(&s); hu[i] = 1.0f + frand(&s); hv[i] = 0.5f + frand(&s); }
    float *dg, *du, *dv, *dout, *dscale;
    double *dws;
    CHECK_HIP(hipMalloc((void **)&dg, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&du, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dv, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dout, sizeof(float) * 3 * N));
    CHECK_HIP(hipMalloc((void **)&dscale, sizeof(float)));
    CHECK_HIP(hipMalloc((void **)&dws, sizeof(double) * (PRE_VJP_SUMSQ_WORKSPACE + 1)));
    CHECK_HIP(hipMemcpy(dg, hg, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(du, hu, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dv, hv, sizeof(float) * N, hipMemcpyHostToDevice));
    const float up = 1000.0f, hs = 0.25f;
    CHECK_HIP(hipMemcpy(dscale, &up, sizeof(float), hipMemcpyHostToDevice));
    const int64_t sB = (int64_t)T * X * Y, sT = (int64_t)X * Y, sX = Y;
    pre_field_t fg = {dg, sB, sT, sX, 1};

    /* gg = hs * up * m * g with the crop mask, as the kernels form it on load */
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        const int m = t >= 1 && t <= T - 2 && x >= 1 && x <= X - 2 && y >= 1 && y <= Y - 2;
        const size_t i = at(b, t, x, y);
        gg[i] = m ? (double)hs * up * hg[i] : 0.0;
        gu[i] = gg[i] * hu[i];
        gv[i] = gg[i] * hv[i];
    }

    /* ---- the wave star: out = S^T(gg) */
    const float r2 = 0.25f;
    float Kw[27] = {0};
    Kw[13] = -2.0f + 4.0f * r2; Kw[4] = 1.0f; Kw[22] = 1.5f;      /* t-, t+ (unequal: the mirroring shows) */
    Kw[10] = -r2; Kw[16] = -0.5f * r2; Kw[12] = -r2; Kw[14] = -2.0f * r2;
    float tw[7];
    int32_t toff[21];
    {
        const int idx[7] = {13, 4, 22, 10, 16, 12, 14};
        for (int k = 0; k < 7; ++k) {
            tw[k] = Kw[idx[k]];
            toff[3 * k] = idx[k] / 9 - 1; toff[3 * k + 1] = idx[k] / 3 % 3 - 1; toff[3 * k + 2] = idx[k] % 3 - 1;
        }
    }
    pre_out_t o0 = {dout, sB, sT, sX, 1};
    int rc = pre_vjp_stencil3d_f32(&fg, &o0, tw, toff, 7, hs, dscale, B, T, X, Y, PRE_VJP_CROP, NULL);
    EXPECT(rc == PRE_OK, "pre_vjp_stencil3d_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(ho, dout, sizeof(float) * N, hipMemcpyDeviceToHost));
    double err = 0.0, scale = 0.0;
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        const double want = Dop(Kw, gg, b, t, x, y, -1);
        err = fmax(err, fabs(ho[at(b, t, x, y)] - want));
        scale = fmax(scale, fabs(want));
    }
    printf("      wave VJP max err %.3e of scale %.3e\n", err, scale);
    EXPECT(err <= 1e-5 * scale, "wave-star VJP matches the C loops (crop mask, device scale, odd width)");

    /* ---- NS momentum: three gradients in one launch, into the slots of one [B,3,T,X,Y] buffer */
    float Kt[27] = {0}, Kx[27] = {0}, Ky[27] = {0}, KL[27] = {0};
    Kt[4] = -1.0f; Kt[22] = 1.0f;                                 /* central differences; D_y along Ny here */
    Kx[10] = -1.0f; Kx[16] = 1.0f;
    Ky[12] = -1.0f; Ky[14] = 1.0f;
    KL[13] = -4.0f; KL[10] = KL[16] = KL[12] = KL[14] = 1.0f;
    const float dt = 0.01f, dx = 0.02f, dy = 0.04f, nu = 0.001f;
    const double a = (double)dx * dy, bq = (double)dt * dy, c = (double)dt * dx, n = (double)nu * dt;
    pre_field_t uv[2] = {{du, sB, sT, sX, 1}, {dv, sB, sT, sX, 1}};
    pre_out_t o3[3] = {{dout, 3 * sB, sT, sX, 1}, {dout + sB, 3 * sB, sT, sX, 1}, {dout + 2 * sB, 3 * sB, sT, sX, 1}};
    rc = pre_vjp_ns_momentum_f32(&fg, uv, o3, Kt, Kx, Ky, KL, dt, dx, dy, nu, hs, dscale, B, T, X, Y, PRE_VJP_CROP, NULL);
    EXPECT(rc == PRE_OK, "pre_vjp_ns_momentum_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(ho, dout, sizeof(float) * 3 * N, hipMemcpyDeviceToHost));
    for (int i = 0; i < N; ++i) { du_[i] = hu[i]; dv_[i] = hv[i]; }
    err = 0.0; scale = 0.0;
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        const double g0 = gg[at(b, t, x, y)];
        const double lin = a * Dop(Kt, gg, b, t, x, y, -1) - n * Dop(KL, gg, b, t, x, y, -1);
        const double XT = Dop(Kx, gu, b, t, x, y, -1), YT = Dop(Ky, gv, b, t, x, y, -1);
        const double want[3] = {
            lin + g0 * (bq * Dop(Kx, du_, b, t, x, y, 1) + c * Dop(Kx, dv_, b, t, x, y, 1)) + bq * XT + c * YT,
            lin + g0 * (c * Dop(Ky, du_, b, t, x, y, 1) + bq * Dop(Ky, dv_, b, t, x, y, 1)) + c * XT + bq * YT,
            bq * Dop(Kx, gg, b, t, x, y, -1) + c * Dop(Ky, gg, b, t, x, y, -1)};
        for (int k = 0; k < 3; ++k) {
            const double got = ho[(((size_t)(b * 3 + k) * T + t) * X + x) * Y + y];
            err = fmax(err, fabs(got - want[k]));
            scale = fmax(scale, fabs(want[k]));
        }
    }
    printf("      NS VJP max err %.3e of scale %.3e\n", err, scale);
    EXPECT(err <= 1e-5 * scale, "NS momentum VJP (du, dv, dp in one launch) matches the C loops");

    /* ---- sum(m * g^2), twice: the same bits */
    double sums[2], want = 0.0;
    for (int rep = 0; rep < 2; ++rep) {
        rc = pre_vjp_sumsq_f32(&fg, B, T, X, Y, PRE_VJP_CROP, dws, dws + PRE_VJP_SUMSQ_WORKSPACE, NULL);
        CHECK_HIP(hipDeviceSynchronize());
        CHECK_HIP(hipMemcpy(&sums[rep], dws + PRE_VJP_SUMSQ_WORKSPACE, sizeof(double), hipMemcpyDeviceToHost));
    }
    for (int b = 0; b < B; ++b) for (int t = 1; t < T - 1; ++t) for (int x = 1; x < X - 1; ++x) for (int y = 1; y < Y - 1; ++y)
        want += (double)hg[at(b, t, x, y)] * hg[at(b, t, x, y)];
    EXPECT(rc == PRE_OK && fabs(sums[0] - want) <= 1e-12 * want, "pre_vjp_sumsq_f32 matches the fp64 loop");
    EXPECT(memcmp(&sums[0], &sums[1], sizeof(double)) == 0, "pre_vjp_sumsq_f32 twice: the same bits");

    /* ---- argument errors: nothing is launched */
    EXPECT(pre_vjp_stencil3d_f32(NULL, &o0, tw, toff, 7, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null g -> PRE_E_NULL");
    EXPECT(pre_vjp_stencil3d_f32(&fg, &o0, tw, toff, 7, 1.0f, NULL, B, 0, X, Y, 0, NULL) == PRE_E_NULL, "empty extent -> PRE_E_NULL");
    pre_out_t alias = {dg, sB, sT, sX, 1};
    EXPECT(pre_vjp_stencil3d_f32(&fg, &alias, tw, toff, 7, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_SHAPE, "out overlapping g -> PRE_E_SHAPE");
    const int32_t box[3] = {1, 1, 0};
    EXPECT(pre_vjp_stencil3d_f32(&fg, &o0, tw, box, 1, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "tap off the star -> PRE_E_UNSUPPORTED");
    float Kbox[27] = {0};
    Kbox[0] = 1.0f;
    EXPECT(pre_vjp_ns_momentum_f32(&fg, uv, o3, Kt, Kbox, Ky, KL, dt, dx, dy, nu, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED,
           "NS: kernel off the star -> PRE_E_UNSUPPORTED");
    pre_out_t o3a[3] = {o3[0], {du, sB, sT, sX, 1}, o3[2]};
    EXPECT(pre_vjp_ns_momentum_f32(&fg, uv, o3a, Kt, Kx, Ky, KL, dt, dx, dy, nu, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_SHAPE,
           "NS: an output overlapping u -> PRE_E_SHAPE");
    EXPECT(pre_vjp_ns_momentum_f32(&fg, NULL, o3, Kt, Kx, Ky, KL, dt, dx, dy, nu, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "NS: null fields");
    pre_field_t tfast = {dg, sB, 1, (int64_t)T * Y, T};
    EXPECT(pre_vjp_stencil3d_f32(&tfast, &o0, tw, toff, 7, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "Nt-fastest view -> PRE_E_UNSUPPORTED");
    pre_out_t o2[2] = {o3[0], o3[1]};
    EXPECT(pre_vjp_linear2_f32(&fg, o2, Kx, NULL, 1.0f, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "linear2: null kernel");
    const int64_t st3[3] = {(int64_t)X * Y, Y, 1};
    float K9[9] = {0};
    EXPECT(pre_vjp_burgers_f32(dg, st3, du, st3, du, st3, K9, K9, K9, 0.1f, 0.1f, 0.1f, 0.1f, 1.0f, NULL, T, X, Y, 0, NULL) == PRE_E_SHAPE,
           "burgers: du aliasing u -> PRE_E_SHAPE");
    EXPECT(pre_vjp_stencil2d_f32(dg, st3, NULL, st3, tw, toff, 0, 1.0f, NULL, T, X, Y, 0, NULL) == PRE_E_NULL, "stencil2d: null out");
    EXPECT(pre_vjp_sumsq_f32(&fg, B, T, X, Y, 0, NULL, dws, NULL) == PRE_E_NULL, "sumsq: null workspace");
    hipFree(dg); hipFree(du); hipFree(dv); hipFree(dout); hipFree(dscale); hipFree(dws);
    free(hg); free(hu); free(hv); free(ho); free(gg); free(gu); free(gv); free(du_); free(dv_);
    return failures ? 1 : 0;
}
