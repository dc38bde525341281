/* A C99 client of libcp_pre_screenbc.so (cp_pre_screenbc.h): a star operator with taps along Nt on a [3,3,7,8] field under
 * a true wrap in y, the constant 2.5 above row 0 and a reflection below the last row (planes t = -1 and t = T are zero, their
 * padded ring included), screened against two levels with a modulation and reduced to its per-sample statistics, both over
 * the whole plane (crop 0, 0, 0), against sums evaluated in this program in double; and the argument errors the entries
 * return before any device work.  Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/screenbc_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_screenbc.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o screenbc_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_screenbc.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 3, T = 3, X = 7, Y = 8, P = T * X * Y, N = B * P, NK = 2 };

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f + 0.5f; }

static const float *H;

/* cell (t, x, y) of sample b under the conditions of main(): -1 <= t <= T, -1 <= x <= X, -1 <= y <= Y */
static double cell(int b, int t, int x, int y)
{
    if (t < 0 || t >= T) return 0.0;
    if (x < 0) return 2.5;
    if (x >= X) x = X - 2;
    if (y < 0) y = Y - 1;
    if (y >= Y) y = 0;
    return (double)H[((b * T + t) * X + x) * Y + y];
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_screenbc_abi_version() == PRE_SCREENBC_ABI_VERSION, "pre_screenbc_abi_version");
    EXPECT(pre_screenbc_stats_workspace_len(B, T, X, Y) == 3 * B && pre_screenbc_stats_workspace_len(B, T, X, 0) == 0 &&
           pre_screenbc_stats_workspace_len(2, 17, 9, 260) == 3 * 2 * 2 * 2 * 3, "pre_screenbc_stats_workspace_len (host only)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    /* the star as a tap list: centre, t-, t+, x-, x+, y-, y+ */
    const float w[7] = {-1.25f, 0.5f, -0.75f, 2.0f, -3.0f, 0.25f, 1.5f};
    const int32_t off[21] = {0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1};
    const pre_bc_t bc = {{PRE_BC_PERIODIC, PRE_BC_PERIODIC, PRE_BC_CONSTANT, PRE_BC_REFLECT}, {0, 0, 2.5f, 0}};

    float *hv = malloc(sizeof(float) * N), hm[P];
    double *r = malloc(sizeof(double) * N);
    unsigned seed = 11u;
    for (int i = 0; i < N; ++i) hv[i] = frand(&seed) * (1.0f + 0.5f * (float)(i / P));      /* the samples' scores lie apart */
    for (int i = 0; i < P; ++i) hm[i] = 0.5f + frand(&seed);
    H = hv;
    double top = 0.0, score[B], mmin = 1e30;
    for (int i = 0; i < P; ++i) mmin = fmin(mmin, (double)hm[i]);
    for (int b = 0; b < B; ++b) {
        score[b] = 0.0;
        for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
            const double v = (double)w[0] * cell(b, t, x, y) + (double)w[1] * cell(b, t - 1, x, y) + (double)w[2] * cell(b, t + 1, x, y) +
                             (double)w[3] * cell(b, t, x - 1, y) + (double)w[4] * cell(b, t, x + 1, y) +
                             (double)w[5] * cell(b, t, x, y - 1) + (double)w[6] * cell(b, t, x, y + 1);
            r[((b * T + t) * X + x) * Y + y] = v;
            top = fmax(top, fabs(v));
            score[b] = fmax(score[b], fabs(v) / (double)hm[(t * X + x) * Y + y]);
        }
    }
    const double tau = 1e-5 * top;
    /* one level between the two lowest scores, one below every score */
    double lo = fmin(score[0], fmin(score[1], score[2])), hi = fmax(score[0], fmax(score[1], score[2]));
    double mid = score[0] + score[1] + score[2] - lo - hi;
    const float hq[NK] = {(float)(0.4 * lo), (float)(0.5 * (lo + mid))};
    long want[NK][B], slack[NK][B];
    for (int k = 0; k < NK; ++k) for (int b = 0; b < B; ++b) {
        want[k][b] = slack[k][b] = 0;
        for (int i = 0; i < P; ++i) {
            const double d = fabs(r[b * P + i]) - (double)hq[k] * (double)hm[i];
            want[k][b] += d <= 0.0;
            slack[k][b] += fabs(d) <= tau;
        }
    }

    float *dv, *dm, *dq;
    uint32_t *dscore, *dcount, *dmax;
    double *dsums, *dws;
    const int64_t wslen = pre_screenbc_stats_workspace_len(B, T, X, Y);
    CHECK_HIP(hipMalloc((void **)&dv, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dm, sizeof hm));
    CHECK_HIP(hipMalloc((void **)&dq, sizeof hq));
    CHECK_HIP(hipMalloc((void **)&dscore, sizeof(uint32_t) * B));
    CHECK_HIP(hipMalloc((void **)&dcount, sizeof(uint32_t) * NK * B));
    CHECK_HIP(hipMalloc((void **)&dmax, sizeof(uint32_t) * B));
    CHECK_HIP(hipMalloc((void **)&dsums, sizeof(double) * 3 * B));
    CHECK_HIP(hipMalloc((void **)&dws, sizeof(double) * (size_t)wslen));
    CHECK_HIP(hipMemcpy(dv, hv, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dm, hm, sizeof hm, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dq, hq, sizeof hq, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dscore, 0, sizeof(uint32_t) * B));
    CHECK_HIP(hipMemset(dcount, 0, sizeof(uint32_t) * NK * B));
    CHECK_HIP(hipMemset(dmax, 0, sizeof(uint32_t) * B));
    CHECK_HIP(hipMemset(dsums, 0, sizeof(double) * 3 * B));
    CHECK_HIP(hipMemset(dws, 0xff, sizeof(double) * (size_t)wslen));       /* NaN: every slot read is written first */
    const pre_field_t in = {dv, P, X * Y, Y, 1};
    const pre_screen_t s = {dq, NK, dm, X * Y, Y, 0, 0, 0, dscore, dcount, B};
    const pre_screenstats_t st = {0, 0, 0, dmax, dsums, B, dws, wslen};
    EXPECT(pre_screenbc_stencil3d_f32(&in, w, off, 7, &s, &bc, B, T, X, Y, 0, NULL) == PRE_OK, "pre_screenbc_stencil3d_f32 returns PRE_OK");
    EXPECT(pre_screenbc_stats_stencil3d_f32(&in, w, off, 7, &st, &bc, B, T, X, Y, 0, NULL) == PRE_OK,
           "pre_screenbc_stats_stencil3d_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    float gscore[B], gmax[B];
    uint32_t gcount[NK * B];
    double gsums[3 * B];
    CHECK_HIP(hipMemcpy(gscore, dscore, sizeof gscore, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(gcount, dcount, sizeof gcount, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(gmax, dmax, sizeof gmax, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(gsums, dsums, sizeof gsums, hipMemcpyDeviceToHost));
    int ok_score = 1, ok_count = 1, ok_stats = 1;
    for (int b = 0; b < B; ++b) {
        double sum = 0.0, sabs = 0.0, ssq = 0.0, mx = 0.0;
        for (int i = 0; i < P; ++i) { const double v = r[b * P + i]; sum += v; sabs += fabs(v); ssq += v * v; mx = fmax(mx, fabs(v)); }
        printf("      sample %d: score %.7g (double %.7g), max %.7g (%.7g), mean %.7g (%.7g), mean |r| %.7g (%.7g)\n", b,
               (double)gscore[b], score[b], (double)gmax[b], mx, gsums[b] / P, sum / P, gsums[B + b] / P, sabs / P);
        ok_score = ok_score && fabs((double)gscore[b] - score[b]) <= tau / mmin + 1.2e-7 * score[b];
        ok_stats = ok_stats && fabs((double)gmax[b] - mx) <= tau + 1.2e-7 * mx && fabs(gsums[b] - sum) <= tau * P &&
                   fabs(gsums[B + b] - sabs) <= tau * P && fabs(gsums[2 * B + b] - ssq) <= tau * (2.0 * top + tau) * P;
        for (int k = 0; k < NK; ++k) ok_count = ok_count && labs((long)gcount[k * B + b] - want[k][b]) <= slack[k][b];
    }
    EXPECT(ok_score, "score within tau / m_min + one ulp of max |r| / m in double");
    EXPECT(ok_count, "counts within the cells that lie within tau of a level's edge");
    EXPECT(ok_stats, "statistics within tau (per cell) of the sums in double");

    /* ---- argument errors: nothing is launched, the verdicts keep their sentinel */
    CHECK_HIP(hipMemset(dscore, 0x55, sizeof(uint32_t) * B));
    CHECK_HIP(hipMemset(dmax, 0x55, sizeof(uint32_t) * B));
#define CALL(IN, WW, SS, BCP, XX, YY, FL) pre_screenbc_stencil3d_f32(IN, WW, off, 7, SS, BCP, B, T, XX, YY, FL, NULL)
#define SCALL(IN, SS, BCP, XX, YY, FL) pre_screenbc_stats_stencil3d_f32(IN, w, off, 7, SS, BCP, B, T, XX, YY, FL, NULL)
    EXPECT(CALL(NULL, w, &s, &bc, X, Y, 0) == PRE_E_NULL, "null field -> PRE_E_NULL");
    EXPECT(CALL(&in, NULL, &s, &bc, X, Y, 0) == PRE_E_NULL, "null taps -> PRE_E_NULL");
    EXPECT(CALL(&in, w, NULL, &bc, X, Y, 0) == PRE_E_NULL, "null descriptor -> PRE_E_NULL");
    EXPECT(CALL(&in, w, &s, NULL, X, Y, 0) == PRE_E_NULL && SCALL(&in, &st, NULL, X, Y, 0) == PRE_E_NULL, "null bc -> PRE_E_NULL");
    pre_screenstats_t shortws = st;
    shortws.workspace_len = wslen - 1;
    EXPECT(SCALL(&in, &shortws, &bc, X, Y, 0) == PRE_E_NULL, "a workspace shorter than the query's answer -> PRE_E_NULL");
    pre_bc_t bad = bc;
    bad.mode[1] = 7;
    EXPECT(CALL(&in, w, &s, &bad, X, Y, 0) == PRE_E_RANGE && SCALL(&in, &st, &bad, X, Y, 0) == PRE_E_RANGE, "unknown boundary mode -> PRE_E_RANGE");
    EXPECT(CALL(&in, w, &s, &bc, 1, Y, 0) == PRE_E_RANGE, "X < 2 under PRE_BC_REFLECT -> PRE_E_RANGE");
    pre_field_t far = in;
    far.sX = (int64_t)1 << 30;
    EXPECT(CALL(&far, w, &s, &bc, X, Y, 0) == PRE_E_RANGE, "in-plane offsets beyond 32 bits -> PRE_E_RANGE");
    EXPECT(CALL(&in, w, &s, &bc, X, 6, 0) == PRE_E_UNSUPPORTED && SCALL(&in, &st, &bc, X, 6, 0) == PRE_E_UNSUPPORTED, "Y % 4 != 0 -> PRE_E_UNSUPPORTED");
    pre_field_t strided = in;
    strided.sY = 2;
    EXPECT(CALL(&strided, w, &s, &bc, X, 4, 0) == PRE_E_UNSUPPORTED, "no unit stride on Ny -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(&in, w, &s, &bc, X, Y, PRE_FLAG_HALO_X) == PRE_E_UNSUPPORTED && SCALL(&in, &st, &bc, X, Y, PRE_FLAG_HALO_X) == PRE_E_UNSUPPORTED,
           "PRE_FLAG_HALO_X -> PRE_E_UNSUPPORTED");
    const float wbox[2] = {1.0f, 0.5f};
    const int32_t obox[6] = {0, 0, 0, 0, 1, 1};
    EXPECT(pre_screenbc_stencil3d_f32(&in, wbox, obox, 2, &s, &bc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "a tap off the star -> PRE_E_UNSUPPORTED");
    float K[27], G[27];
    memset(K, 0, sizeof K);
    K[13] = 1.0f;
    memcpy(G, K, sizeof G);
    G[4] = G[10] = G[12] = 1.0f;               /* weight on all three axes: the general star */
    pre_field_t six[6];
    for (int i = 0; i < 6; ++i) six[i] = in;
    EXPECT(pre_screenbc_mhd_f32(4, six, K, K, K, 5.0 / 3.0, &s, &bc, B, T, X, Y, 0, NULL) == PRE_E_RANGE &&
           pre_screenbc_stats_mhd_f32(-1, six, K, K, K, 5.0 / 3.0, &st, &bc, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "eq outside [0, 3] -> PRE_E_RANGE");
    EXPECT(pre_screenbc_mhd_f32(1, six, K, G, K, 5.0 / 3.0, &s, &bc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED &&
           pre_screenbc_mhd_f32(2, six, K, G, K, 5.0 / 3.0, &s, &bc, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED,
           "the general star of MHD momentum / energy is not built -> PRE_E_UNSUPPORTED");
    CHECK_HIP(hipDeviceSynchronize());
    uint32_t sent[2 * B];
    CHECK_HIP(hipMemcpy(sent, dscore, sizeof(uint32_t) * B, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(sent + B, dmax, sizeof(uint32_t) * B, hipMemcpyDeviceToHost));
    int intact = 1;
    for (int i = 0; i < 2 * B; ++i) intact = intact && sent[i] == 0x55555555u;
    EXPECT(intact, "no refused call wrote a verdict");
    hipFree(dv); hipFree(dm); hipFree(dq); hipFree(dscore); hipFree(dcount); hipFree(dmax); hipFree(dsums); hipFree(dws);
    free(hv); free(r);
    return failures ? 1 : 0;
}
