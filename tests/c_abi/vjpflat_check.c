/* A C99 client of libcp_pre_vjpflat.so: the vector-Jacobian product of an asymmetric 7-point star on a tiny Nt-fastest grid
 * (memory [B,X,Y,T]), checked against plain C loops on the logical axes (the formulas of cp_pre_vjp.h;
 * Physics_Informed/Wave_FNO_PISL.py:209-217), plus the argument errors the entries return before any device work.
 * Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/vjpflat_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_vjpflat.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o vjpflat_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "cp_pre_vjpflat.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 2, T = 10, X = 7, Y = 6, N = B * T * X * Y };     /* T % 4 = 2: quads straddle row ends; Y*T = 60 */

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f - 0.5f; }

static int inside(int t, int x, int y) { return t >= 0 && t < T && x >= 0 && x < X && y >= 0 && y < Y; }
static size_t at(int b, int t, int x, int y) { return (((size_t)b * X + x) * Y + y) * T + t; }      /* memory [B,X,Y,T] */
static double cell(const double *f, int b, int t, int x, int y) { return inside(t, x, y) ? f[at(b, t, x, y)] : 0.0; }

int main(void)
{
    int failures = 0;
    EXPECT(pre_vjpflat_abi_version() == PRE_VJPFLAT_ABI_VERSION, "pre_vjpflat_abi_version");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    float *hg = malloc(sizeof(float) * N), *ho = malloc(sizeof(float) * N);
    double *gg = malloc(sizeof(double) * N);
    unsigned s = 7u;
    for (int i = 0; i < N; ++i) hg[i] = frand(&s);
    float *dg, *dout, *dscale;
    CHECK_HIP(hipMalloc((void **)&dg, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dout, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dscale, sizeof(float)));
    CHECK_HIP(hipMemcpy(dg, hg, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dout, 0, sizeof(float) * N));
    const float up = 1000.0f, hs = 0.25f;
    CHECK_HIP(hipMemcpy(dscale, &up, sizeof(float), hipMemcpyHostToDevice));
    const int64_t sB = (int64_t)X * Y * T, sX = (int64_t)Y * T, sY = T;
    pre_field_t fg = {dg, sB, 1, sX, sY};
    pre_out_t o0 = {dout, sB, 1, sX, sY};

    /* gg = hs * up * m * g with the crop mask, as the kernel forms it on load */
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        const int m = t >= 1 && t <= T - 2 && x >= 1 && x <= X - 2 && y >= 1 && y <= Y - 2;
        gg[at(b, t, x, y)] = m ? (double)hs * up * hg[at(b, t, x, y)] : 0.0;
    }
    /* an asymmetric star: a mirrored or mis-relabelled tap shows */
    const float tw[7] = {-1.75f, 0.5f, -1.25f, 0.875f, -0.375f, 1.5f, -0.625f};
    const int32_t toff[21] = {0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1};
    int rc = pre_vjpflat_stencil3d_f32(&fg, &o0, tw, toff, 7, hs, dscale, B, T, X, Y, PRE_VJP_CROP, NULL);
    EXPECT(rc == PRE_OK, "pre_vjpflat_stencil3d_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(ho, dout, sizeof(float) * N, hipMemcpyDeviceToHost));
    double err = 0.0, scale = 0.0;
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        double want = 0.0;                                   /* S^T(gg)(p) = sum_k w_k gg(p - k) */
        for (int k = 0; k < 7; ++k) want += (double)tw[k] * cell(gg, b, t - toff[3 * k], x - toff[3 * k + 1], y - toff[3 * k + 2]);
        err = fmax(err, fabs(ho[at(b, t, x, y)] - want));
        scale = fmax(scale, fabs(want));
    }
    printf("      star VJP max err %.3e of scale %.3e\n", err, scale);
    EXPECT(scale > 0.0 && err <= 1e-5 * scale, "Nt-fastest star VJP matches the C loops (crop mask, device scale, straddling quads)");

    /* ---- argument errors: nothing is launched */
    EXPECT(pre_vjpflat_stencil3d_f32(NULL, &o0, tw, toff, 7, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null g -> PRE_E_NULL");
    EXPECT(pre_vjpflat_stencil3d_f32(&fg, &o0, tw, toff, 7, 1.0f, NULL, B, 0, X, Y, 0, NULL) == PRE_E_NULL, "empty extent -> PRE_E_NULL");
    pre_out_t alias = {dg, sB, 1, sX, sY};
    EXPECT(pre_vjpflat_stencil3d_f32(&fg, &alias, tw, toff, 7, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_SHAPE, "out overlapping g -> PRE_E_SHAPE");
    const int32_t box[3] = {1, 1, 0};
    EXPECT(pre_vjpflat_stencil3d_f32(&fg, &o0, tw, box, 1, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "tap off the star -> PRE_E_UNSUPPORTED");
    pre_field_t yfast = {dg, (int64_t)T * X * Y, (int64_t)X * Y, Y, 1};
    EXPECT(pre_vjpflat_stencil3d_f32(&yfast, &o0, tw, toff, 7, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "unit-stride last axis -> PRE_E_UNSUPPORTED");
    pre_field_t pitched = {dg, sB, 1, sX, sY + 2};
    EXPECT(pre_vjpflat_stencil3d_f32(&pitched, &o0, tw, toff, 7, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "rows not dense -> PRE_E_UNSUPPORTED");
    EXPECT(pre_vjpflat_stencil3d_f32(&fg, &o0, tw, toff, 7, 1.0f, NULL, B, 96, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "T = 96 -> PRE_E_UNSUPPORTED");
    float K[27] = {0};
    pre_out_t o2[2] = {o0, o0};
    EXPECT(pre_vjpflat_linear2_f32(&fg, o2, K, NULL, 1.0f, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "linear2: null kernel");
    EXPECT(pre_vjpflat_linear2_f32(&fg, o2, K, K, 1.0f, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_SHAPE, "linear2: two outputs at one address");
    pre_out_t o3[3] = {o0, o0, o0};
    EXPECT(pre_vjpflat_ns_momentum_f32(&fg, NULL, o3, K, K, K, K, 0.1f, 0.1f, 0.1f, 0.1f, 1.0f, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "NS: null fields");
    hipFree(dg); hipFree(dout); hipFree(dscale);
    free(hg); free(ho); free(gg);
    return failures ? 1 : 0;
}
