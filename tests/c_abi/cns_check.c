/* A C99 client of libcp_pre_cns.so: the compressible-NS right-hand side (cp_pre_cns.h; Active_Learning/CNS.py:18-31) of a
 * [2,4,8,16] state under the boundary mapping 'periodic' on all sides gives (low side: the opposite edge; high side: the
 * last cell itself), checked against the expression evaluated in this program in double; the integrator epilogue, in place;
 * and the argument errors the entry returns before any device work.  Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/cns_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_cns.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o cns_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_cns.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 2, C = 4, X = 8, Y = 16, PLANE = X * Y, N = B * C * PLANE };

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f + 0.5f; }

static const float *H;                                 /* the host copy of vars [B,C,X,Y] */

/* cell (x, y) of channel c of sample b, -1 <= x <= X, -1 <= y <= Y */
static double cell(int b, int c, int x, int y)
{
    if (x < 0) x = X - 1;
    if (x >= X) x = X - 1;
    if (y < 0) y = Y - 1;
    if (y >= Y) y = Y - 1;
    return (double)H[((b * C + c) * X + x) * Y + y];
}

static double star(const float *K, int b, int c, int x, int y)
{
    return (double)K[4] * cell(b, c, x, y) + (double)K[1] * cell(b, c, x - 1, y) + (double)K[7] * cell(b, c, x + 1, y) +
           (double)K[3] * cell(b, c, x, y - 1) + (double)K[5] * cell(b, c, x, y + 1);
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_cns_abi_version() == PRE_CNS_ABI_VERSION, "pre_cns_abi_version");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    const float s1 = 1.0f / 0.0078f, s2 = 1.0f / (0.0078f * 0.0078f), gamma = 5.0f / 3.0f, step = 1e-4f;
    /* distinct crosses: a caller's kernels, not the constructor's */
    const float Kgx[9] = {0, -0.5f * s1, 0, 0, 0, 0, 0, 0.5f * s1, 0}, Kgy[9] = {0, 0, 0, -0.25f * s1, 0.125f, 0.75f * s1, 0, 0, 0};
    const float Kdx[9] = {0, -0.5f * s1, 0, 0.5f, 1.0f, 0, 0, 0.5f * s1, 0}, Kdy[9] = {0, 2.0f, 0, -0.5f * s1, 0, 0.5f * s1, 0, -1.0f, 0};
    const float Klap[9] = {0, s2, 0, s2, -4.0f * s2, s2, 0, s2, 0};
    const pre_bc_t bc = {{PRE_BC_PERIODIC, PRE_BC_REPLICATE, PRE_BC_PERIODIC, PRE_BC_REPLICATE}, {0, 0, 0, 0}};

    float *hv = malloc(sizeof(float) * N), *ho = malloc(sizeof(float) * N), *hs = malloc(sizeof(float) * N);
    double *want = malloc(sizeof(double) * N);
    unsigned seed = 11u;
    for (int i = 0; i < N; ++i) hv[i] = frand(&seed);
    H = hv;
    double top[4] = {0, 0, 0, 0};
    for (int b = 0; b < B; ++b) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        const double rho = cell(b, 0, x, y), u = cell(b, 1, x, y), v = cell(b, 2, x, y), p = cell(b, 3, x, y);
        const double div = star(Kdx, b, 1, x, y) + star(Kdy, b, 2, x, y);
        const double dot_rho = u * star(Kgx, b, 0, x, y) + v * star(Kgy, b, 0, x, y);
        const double dot_u = u * star(Kgx, b, 1, x, y) + v * star(Kgy, b, 1, x, y);
        const double dot_v = u * star(Kgx, b, 2, x, y) + v * star(Kgy, b, 2, x, y);
        const double adv = -dot_u - dot_v + star(Klap, b, 1, x, y);
        const double r[4] = {-rho * div - dot_rho, adv + star(Kgx, b, 3, x, y) / rho, adv + star(Kgy, b, 3, x, y) / rho,
                             -(double)gamma * p * div - dot_rho};
        for (int c = 0; c < C; ++c) {
            want[((b * C + c) * X + x) * Y + y] = r[c];
            top[c] = fmax(top[c], fabs(r[c]));
        }
    }

    float *dv, *dout, *dstate;
    CHECK_HIP(hipMalloc((void **)&dv, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dout, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dstate, sizeof(float) * N));
    CHECK_HIP(hipMemcpy(dv, hv, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dstate, hv, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dout, 0xff, sizeof(float) * N));
    pre_cns_plane_t in[4], add[4];
    pre_cns_out_t out[4], state[4];
    for (int c = 0; c < C; ++c) {
        in[c].ptr = dv + c * PLANE; in[c].sB = C * PLANE; in[c].sX = Y;
        out[c].ptr = dout + c * PLANE; out[c].sB = C * PLANE; out[c].sX = Y;
        add[c].ptr = dstate + c * PLANE; add[c].sB = C * PLANE; add[c].sX = Y;
        state[c].ptr = dstate + c * PLANE; state[c].sB = C * PLANE; state[c].sX = Y;
    }

    EXPECT(pre_cns_rhs_f32(in, out, Kgx, Kgy, Kdx, Kdy, Klap, &bc, gamma, NULL, 0.0f, B, X, Y, 0, NULL) == PRE_OK, "pre_cns_rhs_f32 returns PRE_OK");
    EXPECT(pre_cns_rhs_f32(in, state, Kgx, Kgy, Kdx, Kdy, Klap, &bc, gamma, add, step, B, X, Y, 0, NULL) == PRE_OK,
           "pre_cns_rhs_f32 with the epilogue, out == add_to, returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(ho, dout, sizeof(float) * N, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(hs, dstate, sizeof(float) * N, hipMemcpyDeviceToHost));
    double worst = 0.0, worst_step = 0.0;
    for (int i = 0; i < N; ++i) {
        const int c = (i / PLANE) % C;
        worst = fmax(worst, fabs((double)ho[i] - want[i]) / top[c]);
        worst_step = fmax(worst_step, fabs((double)hs[i] - ((double)hv[i] + (double)step * want[i])) / (1.5 + (double)step * top[c]));
    }
    printf("      worst channel-scale error: rhs %.3e, step %.3e\n", worst, worst_step);
    EXPECT(worst <= 1e-5, "rhs matches the expression in double within 1e-5 of each channel's scale");
    EXPECT(worst_step <= 1e-5, "add_to + step * rhs, in place, matches within 1e-5");

    /* ---- argument errors: nothing is launched, out keeps its sentinel */
    CHECK_HIP(hipMemset(dout, 0x55, sizeof(float) * N));
#define CALL(IN, OUT, KGX, BCP, ADD, XX, YY, FL) pre_cns_rhs_f32(IN, OUT, KGX, Kgy, Kdx, Kdy, Klap, BCP, gamma, ADD, step, B, XX, YY, FL, NULL)
    EXPECT(CALL(NULL, out, Kgx, &bc, NULL, X, Y, 0) == PRE_E_NULL, "null in -> PRE_E_NULL");
    EXPECT(CALL(in, out, NULL, &bc, NULL, X, Y, 0) == PRE_E_NULL, "null kernel -> PRE_E_NULL");
    EXPECT(CALL(in, out, Kgx, NULL, NULL, X, Y, 0) == PRE_E_NULL, "null bc -> PRE_E_NULL");
    pre_cns_plane_t hole[4];
    memcpy(hole, in, sizeof hole);
    hole[2].ptr = NULL;
    EXPECT(CALL(hole, out, Kgx, &bc, NULL, X, Y, 0) == PRE_E_NULL, "null plane -> PRE_E_NULL");
    EXPECT(CALL(in, out, Kgx, &bc, NULL, X, 6, 0) == PRE_E_UNSUPPORTED, "Y % 4 != 0 -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(in, out, Kgx, &bc, NULL, 1, Y, 0) == PRE_E_UNSUPPORTED, "X < 2 -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(in, out, Kgx, &bc, NULL, X, Y, 1) == PRE_E_UNSUPPORTED, "unknown flag -> PRE_E_UNSUPPORTED");
    pre_cns_plane_t off[4];
    memcpy(off, in, sizeof off);
    off[1].ptr = in[1].ptr + 1;
    EXPECT(CALL(off, out, Kgx, &bc, NULL, X, 12, 0) == PRE_E_UNSUPPORTED, "a plane base off by one float -> PRE_E_UNSUPPORTED");
    memcpy(off, in, sizeof off);
    off[3].sX = Y + 2;
    EXPECT(CALL(off, out, Kgx, &bc, NULL, 4, Y, 0) == PRE_E_UNSUPPORTED, "a row stride that is no multiple of 4 -> PRE_E_UNSUPPORTED");
    float Kbad[9];
    memcpy(Kbad, Kgx, sizeof Kbad);
    Kbad[8] = 1.0f;
    EXPECT(CALL(in, out, Kbad, &bc, NULL, X, Y, 0) == PRE_E_UNSUPPORTED, "a kernel off the cross -> PRE_E_UNSUPPORTED");
    pre_bc_t bad = bc;
    bad.mode[1] = 7;
    EXPECT(CALL(in, out, Kgx, &bad, NULL, X, Y, 0) == PRE_E_RANGE, "unknown boundary mode -> PRE_E_RANGE");
    pre_cns_out_t onto[4];
    memcpy(onto, out, sizeof onto);
    onto[0].ptr = dv + 3 * PLANE;
    EXPECT(CALL(in, onto, Kgx, &bc, NULL, X, Y, 0) == PRE_E_RANGE, "out on in -> PRE_E_RANGE");
    pre_cns_plane_t shifted[4];
    memcpy(shifted, add, sizeof shifted);
    for (int c = 0; c < C; ++c) shifted[c].ptr = dout + c * PLANE + Y;
    EXPECT(CALL(in, out, Kgx, &bc, shifted, X - 1, Y, 0) == PRE_E_RANGE, "add_to overlapping out without being it -> PRE_E_RANGE");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(ho, dout, sizeof(float) * N, hipMemcpyDeviceToHost));
    int intact = 1;
    for (size_t i = 0; i < sizeof(float) * N; ++i) intact = intact && ((unsigned char *)ho)[i] == 0x55;
    EXPECT(intact, "no refused call wrote out");
    hipFree(dv); hipFree(dout); hipFree(dstate);
    free(hv); free(ho); free(hs); free(want);
    return failures ? 1 : 0;
}
