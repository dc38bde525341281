/* A C99 client of libcp_pre_pair.so: the data-driven score d = r(a) - r(b) of a 7-point stencil over two field sets,
 * checked against plain C loops (Marginal/Wave_Residuals_CP.py:216-219), plus the argument errors every pre_pair_*
 * entry returns before any device work.  Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/pair_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_pair.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -o pair_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "cp_pre_pair.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 2, T = 5, X = 9, Y = 67, N = B * T * X * Y };     /* odd width: the streamed columns and the tail */

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f - 0.5f; }

static float star(const float *f, const float w[7], int b, int t, int x, int y)
{
    /* w = {c, t-, t+, x-, x+, y-, y+}; zero padding */
#define AT(tt, xx, yy) (((tt) < 0 || (tt) >= T || (xx) < 0 || (xx) >= X || (yy) < 0 || (yy) >= Y) ? 0.0 : (double)f[(((b) * T + (tt)) * X + (xx)) * Y + (yy)])
    double acc = w[0] * AT(t, x, y) + w[1] * AT(t - 1, x, y) + w[2] * AT(t + 1, x, y) + w[3] * AT(t, x - 1, y) +
                 w[4] * AT(t, x + 1, y) + w[5] * AT(t, x, y - 1) + w[6] * AT(t, x, y + 1);
#undef AT
    return (float)acc;
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_pair_abi_version() == PRE_PAIR_ABI_VERSION, "pre_pair_abi_version");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    float *ha = malloc(sizeof(float) * N), *hb = malloc(sizeof(float) * N), *hd = malloc(sizeof(float) * N);
    unsigned s = 7u;
    for (int i = 0; i < N; ++i) { ha[i] = frand(&s); hb[i] = ha[i] + 0.25f * frand(&s); }
    float *da, *db, *dd;
    CHECK_HIP(hipMalloc((void **)&da, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&db, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dd, sizeof(float) * N));
    CHECK_HIP(hipMemcpy(da, ha, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(db, hb, sizeof(float) * N, hipMemcpyHostToDevice));
    const int64_t sB = (int64_t)T * X * Y, sT = (int64_t)X * Y, sX = Y;
    pre_field_t fa = {da, sB, sT, sX, 1}, fb = {db, sB, sT, sX, 1};
    pre_out_t o = {dd, sB, sT, sX, 1};
    /* the wave kernel's star: D_tt - r^2 * D_xx_yy */
    const float r2 = 0.25f;
    const float w[7] = {-2.0f + 4.0f * r2, 1.0f, 1.0f, -r2, -r2, -r2, -r2};
    const float tw[7] = {w[1], w[3], w[5], w[0], w[6], w[4], w[2]};
    const int32_t toff[21] = {-1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0};
    int rc = pre_pair_stencil3d_f32(&fa, &fb, &o, tw, toff, 7, B, T, X, Y, PRE_FLAG_ABS, NULL);
    EXPECT(rc == PRE_OK, "pre_pair_stencil3d_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(hd, dd, sizeof(float) * N, hipMemcpyDeviceToHost));
    double err = 0.0, scale = 0.0;
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        const float ra = star(ha, w, b, t, x, y), rb = star(hb, w, b, t, x, y);
        const double e = fabs((double)hd[((b * T + t) * X + x) * Y + y] - fabs((double)ra - (double)rb));
        err = e > err ? e : err;
        scale = fabs(ra) > scale ? fabs(ra) : scale;
        scale = fabs(rb) > scale ? fabs(rb) : scale;
    }
    printf("      |d| max err %.3e of residual scale %.3e\n", err, scale);
    EXPECT(err <= 1e-5 * scale, "|r(a) - r(b)| matches the C loops (odd width: march + tail)");

    /* argument errors: nothing is launched */
    EXPECT(pre_pair_stencil3d_f32(&fa, NULL, &o, tw, toff, 7, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null set -> PRE_E_NULL");
    pre_out_t alias = {db, sB, sT, sX, 1};
    EXPECT(pre_pair_stencil3d_f32(&fa, &fb, &alias, tw, toff, 7, B, T, X, Y, 0, NULL) == PRE_E_SHAPE, "out overlapping an input -> PRE_E_SHAPE");
    const int32_t box[3] = {1, 1, 0};
    EXPECT(pre_pair_stencil3d_f32(&fa, &fb, &o, tw, box, 1, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "tap off the star -> PRE_E_UNSUPPORTED");
    pre_field_t a3[3] = {fa, fa, fa}, b3[3] = {fb, fb, fb};
    float K[27] = {0};
    K[13] = 1.0f;
    EXPECT(pre_pair_ns_momentum_f32(a3, b3, &o, K, K, K, K, 0.1f, 0.1f, 0.1f, 0.001f, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED,
           "fused NS momentum on an odd width -> PRE_E_UNSUPPORTED (as its twin)");
    EXPECT(pre_pair_mhd_continuity_f32(a3, NULL, &o, K, K, K, 5.0 / 3.0, B, T, X, Y, 0, NULL) == PRE_E_NULL, "mhd continuity: null set");
    pre_field_t a2[2] = {fa, fa}, b2[2] = {fb, fb};
    EXPECT(pre_pair_linear2_f32(a2, b2, &o, K, NULL, 1.0f, B, T, X, Y, 0, NULL) == PRE_E_NULL, "linear2: null kernel");
    const int64_t st3[3] = {(int64_t)T * X, X, 1};
    float K9[9] = {0};
    EXPECT(pre_pair_burgers_f32(da, st3, db, st3, da, st3, K9, K9, K9, 0.1f, 0.1f, 0.1f, 0.1f, B, T, X, 0, NULL) == PRE_E_SHAPE,
           "burgers: out aliasing a -> PRE_E_SHAPE");
    EXPECT(pre_pair_stencil2d_f32(da, st3, db, st3, dd, st3, tw, toff, 0, B, T, X, PRE_FLAG_HALO_X, NULL) == PRE_E_UNSUPPORTED,
           "stencil2d: halo_x -> PRE_E_UNSUPPORTED");
    hipFree(da); hipFree(db); hipFree(dd);
    free(ha); free(hb); free(hd);
    return failures ? 1 : 0;
}
