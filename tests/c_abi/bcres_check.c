/* A C99 client of libcp_pre_bcres.so (cp_pre_bcres.h): a star operator with taps along Nt on a [2,3,7,8] field under a true
 * wrap in y, the constant 2.5 above row 0 and a reflection below the last row, checked against the sum evaluated in this
 * program in double (planes t = -1 and t = T are zero, their padded ring included); the Burgers entry on [3,5,8] under a
 * wrap in x; and the argument errors the entries return before any device work.  Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/bcres_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_bcres.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o bcres_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_bcres.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 2, T = 3, X = 7, Y = 8, N = B * T * X * Y, B1 = 3, T1 = 5, X1 = 8, N1 = B1 * T1 * X1 };

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f + 0.5f; }

static const float *H;

/* cell (t, x, y) of sample b under the conditions of main(): -1 <= t <= T, -1 <= x <= X, -1 <= y <= Y */
static double cell(int b, int t, int x, int y)
{
    if (t < 0 || t >= T) return 0.0;               /* the zero padding in time covers the padded ring too */
    if (x < 0) return 2.5;
    if (x >= X) x = X - 2;
    if (y < 0) y = Y - 1;
    if (y >= Y) y = 0;
    return (double)H[((b * T + t) * X + x) * Y + y];
}

static double cell1(const float *u, int b, int t, int x)
{
    if (t < 0 || t >= T1) return 0.0;
    if (x < 0) x = X1 - 1;
    if (x >= X1) x = 0;
    return (double)u[(b * T1 + t) * X1 + x];
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_bcres_abi_version() == PRE_BCRES_ABI_VERSION, "pre_bcres_abi_version");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    /* centre, t-, t+, x-, x+, y-, y+ on the dense 3x3x3 kernel, axes (Nt, Nx, Ny) */
    float K[27];
    memset(K, 0, sizeof K);
    K[13] = -1.25f; K[4] = 0.5f; K[22] = -0.75f; K[10] = 2.0f; K[16] = -3.0f; K[12] = 0.25f; K[14] = 1.5f;
    const pre_bc_t bc = {{PRE_BC_PERIODIC, PRE_BC_PERIODIC, PRE_BC_CONSTANT, PRE_BC_REFLECT}, {0, 0, 2.5f, 0}};

    float *hv = malloc(sizeof(float) * N), *ho = malloc(sizeof(float) * N);
    double *want = malloc(sizeof(double) * N);
    unsigned seed = 5u;
    for (int i = 0; i < N; ++i) hv[i] = frand(&seed);
    H = hv;
    double top = 0.0;
    for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        const double r = (double)K[13] * cell(b, t, x, y) + (double)K[4] * cell(b, t - 1, x, y) + (double)K[22] * cell(b, t + 1, x, y) +
                         (double)K[10] * cell(b, t, x - 1, y) + (double)K[16] * cell(b, t, x + 1, y) +
                         (double)K[12] * cell(b, t, x, y - 1) + (double)K[14] * cell(b, t, x, y + 1);
        want[((b * T + t) * X + x) * Y + y] = r;
        top = fmax(top, fabs(r));
    }
    float *dv, *dout;
    CHECK_HIP(hipMalloc((void **)&dv, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dout, sizeof(float) * N));
    CHECK_HIP(hipMemcpy(dv, hv, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dout, 0xff, sizeof(float) * N));
    pre_field_t in = {dv, T * X * Y, X * Y, Y, 1};
    pre_out_t out = {dout, T * X * Y, X * Y, Y, 1};
    EXPECT(pre_bcres_linear1_f32(&in, &out, K, &bc, B, T, X, Y, 0, NULL) == PRE_OK, "pre_bcres_linear1_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(ho, dout, sizeof(float) * N, hipMemcpyDeviceToHost));
    double worst = 0.0;
    for (int i = 0; i < N; ++i) worst = fmax(worst, fabs((double)ho[i] - want[i]) / top);
    printf("      worst tensor-scale error: linear1 %.3e\n", worst);
    EXPECT(worst <= 1e-5, "the star with t-taps under wrap / constant / reflect matches the sum in double within 1e-5");

    /* ---- Burgers on [B1,T1,X1], a wrap in x; the rows (time) keep the zero padding whatever top / bottom say */
    const float Kt[9] = {0, -1, 0, 0, 0, 0, 0, 1, 0}, Kx[9] = {0, 0, 0, -1, 0, 1, 0, 0, 0}, Kxx[9] = {0, 0, 0, 1, -2, 1, 0, 0, 0};
    const float dx = 0.125f, dt = 0.1f, nu = 0.002f, c3 = 2.0f * dt / dx;
    const pre_bc_t wrap = {{PRE_BC_PERIODIC, PRE_BC_PERIODIC, PRE_BC_REFLECT, PRE_BC_REPLICATE}, {0, 0, 0, 0}};
    float hu[N1], hr[N1];
    for (int i = 0; i < N1; ++i) hu[i] = frand(&seed);
    float *du, *dr;
    CHECK_HIP(hipMalloc((void **)&du, sizeof hu));
    CHECK_HIP(hipMalloc((void **)&dr, sizeof hr));
    CHECK_HIP(hipMemcpy(du, hu, sizeof hu, hipMemcpyHostToDevice));
    const int64_t s1[3] = {T1 * X1, X1, 1};
    EXPECT(pre_bcres_burgers_f32(du, s1, dr, s1, Kt, Kx, Kxx, dx, dt, nu, c3, &wrap, B1, T1, X1, 0, NULL) == PRE_OK,
           "pre_bcres_burgers_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(hr, dr, sizeof hr, hipMemcpyDeviceToHost));
    double worst1 = 0.0, top1 = 0.0, w1[N1];
    for (int b = 0; b < B1; ++b) for (int t = 0; t < T1; ++t) for (int x = 0; x < X1; ++x) {
        const double u = cell1(hu, b, t, x);
        const double r = (double)dx * (cell1(hu, b, t + 1, x) - cell1(hu, b, t - 1, x)) +
                         (double)dt * u * (cell1(hu, b, t, x + 1) - cell1(hu, b, t, x - 1)) -
                         (double)nu * (cell1(hu, b, t, x - 1) - 2.0 * u + cell1(hu, b, t, x + 1)) * (double)c3;
        w1[(b * T1 + t) * X1 + x] = r;
        top1 = fmax(top1, fabs(r));
    }
    for (int i = 0; i < N1; ++i) worst1 = fmax(worst1, fabs((double)hr[i] - w1[i]) / top1);
    printf("      worst tensor-scale error: burgers %.3e\n", worst1);
    EXPECT(worst1 <= 1e-5, "Burgers under a wrap in x matches the expression in double within 1e-5");

    /* ---- argument errors: nothing is launched, out keeps its sentinel */
    CHECK_HIP(hipMemset(dout, 0x55, sizeof(float) * N));
#define CALL(IN, OUT, KK, BCP, XX, YY, FL) pre_bcres_linear1_f32(IN, OUT, KK, BCP, B, T, XX, YY, FL, NULL)
    EXPECT(CALL(NULL, &out, K, &bc, X, Y, 0) == PRE_E_NULL, "null in -> PRE_E_NULL");
    EXPECT(CALL(&in, NULL, K, &bc, X, Y, 0) == PRE_E_NULL, "null out -> PRE_E_NULL");
    EXPECT(CALL(&in, &out, NULL, &bc, X, Y, 0) == PRE_E_NULL, "null kernel -> PRE_E_NULL");
    EXPECT(CALL(&in, &out, K, NULL, X, Y, 0) == PRE_E_NULL, "null bc -> PRE_E_NULL");
    pre_bc_t bad = bc;
    bad.mode[1] = 7;
    EXPECT(CALL(&in, &out, K, &bad, X, Y, 0) == PRE_E_RANGE, "unknown boundary mode -> PRE_E_RANGE");
    EXPECT(CALL(&in, &out, K, &bc, 1, Y, 0) == PRE_E_RANGE, "X < 2 under PRE_BC_REFLECT -> PRE_E_RANGE");
    pre_field_t far = in;
    far.sX = (int64_t)1 << 30;
    EXPECT(CALL(&far, &out, K, &bc, X, Y, 0) == PRE_E_RANGE, "in-plane offsets beyond 32 bits -> PRE_E_RANGE");
    EXPECT(CALL(&in, &out, K, &bc, X, 6, 0) == PRE_E_UNSUPPORTED, "Y % 4 != 0 -> PRE_E_UNSUPPORTED");
    pre_field_t strided = in;
    strided.sY = 2;
    EXPECT(CALL(&strided, &out, K, &bc, X, 4, 0) == PRE_E_UNSUPPORTED, "no unit stride on Ny -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(&in, &out, K, &bc, X, Y, PRE_FLAG_HALO_X) == PRE_E_UNSUPPORTED, "PRE_FLAG_HALO_X -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(&in, &out, K, &bc, X, Y, PRE_FLAG_OUT_INTERIOR_T) == PRE_E_UNSUPPORTED, "PRE_FLAG_OUT_INTERIOR_T -> PRE_E_UNSUPPORTED");
    float Kbad[27];
    memcpy(Kbad, K, sizeof Kbad);
    Kbad[0] = 1.0f;
    EXPECT(CALL(&in, &out, Kbad, &bc, X, Y, 0) == PRE_E_UNSUPPORTED, "a kernel off the star -> PRE_E_UNSUPPORTED");
    pre_field_t six[6];
    for (int i = 0; i < 6; ++i) six[i] = in;
    EXPECT(pre_bcres_mhd_f32(4, six, &out, K, K, K, 5.0 / 3.0, &bc, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "eq outside [0, 3] -> PRE_E_RANGE");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(ho, dout, sizeof(float) * N, hipMemcpyDeviceToHost));
    int intact = 1;
    for (size_t i = 0; i < sizeof(float) * N; ++i) intact = intact && ((unsigned char *)ho)[i] == 0x55;
    EXPECT(intact, "no refused call wrote out");
    hipFree(dv); hipFree(dout); hipFree(du); hipFree(dr);
    free(hv); free(ho); free(want);
    return failures ? 1 : 0;
}
