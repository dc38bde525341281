/* A C99 client of libcp_pre_wgrad.so: the gradient of a residual loss with respect to a dense 3x3x3 operator kernel on a
 * tiny grid, in both layouts the entry takes (Y-fastest, memory [B,T,X,Y], and Nt-fastest, memory [B,X,Y,T]), checked
 * against a plain C double loop (the formula of cp_pre_wgrad.h; Physics_Informed/Wave_FNO_PI.py:202-210), plus the argument
 * errors the entry returns before any device work.  Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/wgrad_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_wgrad.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o wgrad_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_wgrad.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 3, T = 7, X = 9, Y = 6, N = B * T * X * Y };

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f - 0.5f; }
static int inside(int t, int x, int y) { return t >= 0 && t < T && x >= 0 && x < X && y >= 0 && y < Y; }
/* element offset of logical cell (b,t,x,y): layout 0 = memory [B,T,X,Y], 1 = memory [B,X,Y,T] */
static size_t at(int layout, int b, int t, int x, int y)
{
    return layout ? (((size_t)b * X + x) * Y + y) * T + t : (((size_t)b * T + t) * X + x) * Y + y;
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_wgrad_abi_version() == PRE_WGRAD_ABI_VERSION, "pre_wgrad_abi_version");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    float *hg = malloc(sizeof(float) * N), *hx = malloc(sizeof(float) * N), *hy = malloc(sizeof(float) * N), hk[27];
    float *dg, *dx, *dy, *dk, *dscale;
    double *dws;
    CHECK_HIP(hipMalloc((void **)&dg, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dx, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dy, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dk, sizeof(float) * 27));
    CHECK_HIP(hipMalloc((void **)&dscale, sizeof(float)));
    CHECK_HIP(hipMalloc((void **)&dws, sizeof(double) * PRE_WGRAD_WORKSPACE));
    const float up = 1000.0f, hs = 0.25f;
    CHECK_HIP(hipMemcpy(dscale, &up, sizeof(float), hipMemcpyHostToDevice));

    for (int layout = 0; layout < 2; ++layout) {
        unsigned s = 7u + (unsigned)layout;
        for (int i = 0; i < N; ++i) { hg[i] = frand(&s); hx[i] = frand(&s) + 1.0f; hy[i] = frand(&s) + 1.0f; }
        CHECK_HIP(hipMemcpy(dg, hg, sizeof(float) * N, hipMemcpyHostToDevice));
        CHECK_HIP(hipMemcpy(dx, hx, sizeof(float) * N, hipMemcpyHostToDevice));
        CHECK_HIP(hipMemcpy(dy, hy, sizeof(float) * N, hipMemcpyHostToDevice));
        CHECK_HIP(hipMemset(dk, 0xff, sizeof(float) * 27));
        const int64_t sB = (int64_t)T * X * Y;
        const int64_t sT = layout ? 1 : (int64_t)X * Y, sX = layout ? (int64_t)Y * T : Y, sY = layout ? T : 1;
        pre_field_t fg = {dg, sB, sT, sX, sY}, fx = {dx, sB, sT, sX, sY}, fy = {dy, sB, sT, sX, sY};
        int rc = pre_wgrad_stencil3d_f32(&fg, &fx, &fy, 3, 3, 3, hs, dscale, B, T, X, Y, PRE_VJP_CROP, dws, dk, NULL);
        EXPECT(rc == PRE_OK, layout ? "Nt-fastest: pre_wgrad_stencil3d_f32 returns PRE_OK" : "Y-fastest: pre_wgrad_stencil3d_f32 returns PRE_OK");
        CHECK_HIP(hipDeviceSynchronize());
        CHECK_HIP(hipMemcpy(hk, dk, sizeof(float) * 27, hipMemcpyDeviceToHost));
        double worst = 0.0;
        for (int it = 0; it < 3; ++it) for (int ix = 0; ix < 3; ++ix) for (int iy = 0; iy < 3; ++iy) {
            double want = 0.0, S = 0.0;
            for (int b = 0; b < B; ++b) for (int t = 1; t < T - 1; ++t) for (int x = 1; x < X - 1; ++x) for (int y = 1; y < Y - 1; ++y) {
                const int tt = t + it - 1, xx = x + ix - 1, yy = y + iy - 1;
                if (!inside(tt, xx, yy)) continue;
                const double z = (double)hx[at(layout, b, tt, xx, yy)] - (double)hy[at(layout, b, tt, xx, yy)];
                want += (double)hg[at(layout, b, t, x, y)] * z;
                S += fabs((double)hg[at(layout, b, t, x, y)] * z);
            }
            want *= (double)hs * up;
            S *= (double)hs * up;
            const double ratio = fabs(hk[(it * 3 + ix) * 3 + iy] - want) / (36.0 * ldexp(1.0, -24) * S);     /* (L + 4) 2^-24 S */
            worst = fmax(worst, ratio);
        }
        printf("      layout %d: worst |dk - dk64| / bound = %.3f\n", layout, worst);
        EXPECT(worst <= 1.0, layout ? "Nt-fastest dk matches the C loops (crop, x - y, device scale, logical tap order)"
                                    : "Y-fastest dk matches the C loops (crop, x - y, device scale)");
    }

    /* ---- argument errors: nothing is launched, dk keeps its sentinel */
    const int64_t sB = (int64_t)T * X * Y;
    pre_field_t fg = {dg, sB, (int64_t)X * Y, Y, 1}, fx = {dx, sB, (int64_t)X * Y, Y, 1};
    CHECK_HIP(hipMemset(dk, 0x55, sizeof(float) * 27));
    EXPECT(pre_wgrad_stencil3d_f32(NULL, &fx, NULL, 3, 3, 3, 1.0f, NULL, B, T, X, Y, 0, dws, dk, NULL) == PRE_E_NULL, "null g -> PRE_E_NULL");
    EXPECT(pre_wgrad_stencil3d_f32(&fg, &fx, NULL, 3, 3, 3, 1.0f, NULL, B, T, X, Y, 0, NULL, dk, NULL) == PRE_E_NULL, "null workspace -> PRE_E_NULL");
    EXPECT(pre_wgrad_stencil3d_f32(&fg, &fx, NULL, 3, 3, 3, 1.0f, NULL, B, 0, X, Y, 0, dws, dk, NULL) == PRE_E_NULL, "empty extent -> PRE_E_NULL");
    EXPECT(pre_wgrad_stencil3d_f32(&fg, &fx, NULL, 5, 3, 3, 1.0f, NULL, B, T, X, Y, 0, dws, dk, NULL) == PRE_E_UNSUPPORTED, "extent 5 -> PRE_E_UNSUPPORTED");
    EXPECT(pre_wgrad_stencil3d_f32(&fg, &fx, NULL, 3, 3, 3, 1.0f, NULL, B, T, X, Y, 4, dws, dk, NULL) == PRE_E_UNSUPPORTED, "unknown flag -> PRE_E_UNSUPPORTED");
    pre_field_t odd = {dx, sB, (int64_t)X * Y, 1, X};
    EXPECT(pre_wgrad_stencil3d_f32(&fg, &odd, NULL, 3, 3, 3, 1.0f, NULL, B, T, X, Y, 0, dws, dk, NULL) == PRE_E_UNSUPPORTED, "x with unit stride on X -> PRE_E_UNSUPPORTED");
    EXPECT(pre_wgrad_stencil3d_f32(&fg, &fx, NULL, 3, 3, 3, 1.0f, NULL, B, T, X, Y, 0, dws, dx + 5, NULL) == PRE_E_SHAPE, "dk inside x -> PRE_E_SHAPE");
    EXPECT(pre_wgrad_stencil3d_f32(&fg, &fx, NULL, 3, 3, 3, 1.0f, NULL, B, T, X, Y, 0, (double *)dg, dk, NULL) == PRE_E_SHAPE, "workspace on g -> PRE_E_SHAPE");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(hk, dk, sizeof(float) * 27, hipMemcpyDeviceToHost));
    unsigned char want[sizeof(float) * 27];
    memset(want, 0x55, sizeof want);
    EXPECT(memcmp(hk, want, sizeof want) == 0, "no refused call wrote dk");
    hipFree(dg); hipFree(dx); hipFree(dy); hipFree(dk); hipFree(dscale); hipFree(dws);
    free(hg); free(hx); free(hy);
    return failures ? 1 : 0;
}
