/* A C99 client of libcp_pre_cnsvjp.so: the vector-Jacobian product (cp_pre_cnsvjp.h) of the compressible-NS right-hand side of
 * a [2,4,8,16] state, under the boundary mapping of cns_check.c (low side: the opposite edge; high side: the last cell
 * itself) and under a second one with a constant and a reflecting side, checked against the product formed in this program
 * in double the other way round: as a SCATTER of every output cell's derivatives onto the cells its stencils read (the
 * library gathers, with folds); the epilogue with add_to == gin and with add_to == cot; and the argument errors the entry
 * returns before any device work.  Exit code 0 = all ok.
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/cnsvjp_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_cnsvjp.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o cnsvjp_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_cnsvjp.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

enum { B = 2, C = 4, X = 8, Y = 16, PLANE = X * Y, N = B * C * PLANE };

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f + 0.5f; }

static const float *H;                                 /* the host copy of vars [B,C,X,Y] */
static double *G;                                      /* the gradient being scattered [B,C,X,Y] */
static int XLO, XHI, YLO, YHI;                         /* the index read in place of the cell just outside, or -1: the constant */
static double VXLO, VXHI, VYLO, VYHI;

/* (x, y) through the boundary mapping; returns 0 and sets *val for a constant */
static int map(int *x, int *y, double *val)
{
    if (*x < 0) { if (XLO < 0) { *val = VXLO; return 0; } *x = XLO; }
    else if (*x >= X) { if (XHI < 0) { *val = VXHI; return 0; } *x = XHI; }
    if (*y < 0) { if (YLO < 0) { *val = VYLO; return 0; } *y = YLO; }
    else if (*y >= Y) { if (YHI < 0) { *val = VYHI; return 0; } *y = YHI; }
    return 1;
}

static double cell(int b, int c, int x, int y)
{
    double val = 0.0;
    if (!map(&x, &y, &val)) return val;
    return (double)H[((b * C + c) * X + x) * Y + y];
}

static const int DXY[5][2] = {{0, 0}, {-1, 0}, {1, 0}, {0, -1}, {0, 1}};
static const int TAP[5] = {4, 1, 7, 3, 5};             /* dense 3x3 index of the centre, row -1, row +1, column -1, column +1 */

static double star(const float *K, int b, int c, int x, int y)
{
    double s = 0.0;
    for (int t = 0; t < 5; ++t) s += (double)K[TAP[t]] * cell(b, c, x + DXY[t][0], y + DXY[t][1]);
    return s;
}

/* the adjoint of star(): coef * K[t] onto every cell the stencil at (x, y) read in channel c (a constant receives nothing) */
static void scatter(const float *K, int b, int c, int x, int y, double coef)
{
    for (int t = 0; t < 5; ++t) {
        int xx = x + DXY[t][0], yy = y + DXY[t][1];
        double val;
        if (map(&xx, &yy, &val)) G[((b * C + c) * X + xx) * Y + yy] += coef * (double)K[TAP[t]];
    }
}

static void reference(const float *hg, const float *Kgx, const float *Kgy, const float *Kdx, const float *Kdy, const float *Klap,
                      double gamma, double *top)
{
    memset(G, 0, sizeof(double) * N);
    for (int b = 0; b < B; ++b) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) {
        const double rho = cell(b, 0, x, y), u = cell(b, 1, x, y), v = cell(b, 2, x, y), p = cell(b, 3, x, y);
        double g[4];
        for (int c = 0; c < C; ++c) g[c] = (double)hg[((b * C + c) * X + x) * Y + y];
        double *d_rho = &G[((b * C + 0) * X + x) * Y + y], *d_u = d_rho + PLANE, *d_v = d_u + PLANE, *d_p = d_v + PLANE;
        const double div = star(Kdx, b, 1, x, y) + star(Kdy, b, 2, x, y), gm = g[1] + g[2], s = -(g[0] + g[3]);
        const double a = -rho * g[0] - gamma * p * g[3];
        /* mass and energy: -rho*div - (u Ggx rho + v Ggy rho), -gamma*p*div - (the same) */
        *d_rho += -div * g[0];
        *d_p += -gamma * div * g[3];
        scatter(Kdx, b, 1, x, y, a);
        scatter(Kdy, b, 2, x, y, a);
        *d_u += s * star(Kgx, b, 0, x, y);
        *d_v += s * star(Kgy, b, 0, x, y);
        scatter(Kgx, b, 0, x, y, s * u);
        scatter(Kgy, b, 0, x, y, s * v);
        /* both momentum channels: -(u Ggx u + v Ggy u) - (u Ggx v + v Ggy v) + L u */
        *d_u += -gm * (star(Kgx, b, 1, x, y) + star(Kgx, b, 2, x, y));
        *d_v += -gm * (star(Kgy, b, 1, x, y) + star(Kgy, b, 2, x, y));
        scatter(Kgx, b, 1, x, y, -gm * u);
        scatter(Kgy, b, 1, x, y, -gm * v);
        scatter(Kgx, b, 2, x, y, -gm * u);
        scatter(Kgy, b, 2, x, y, -gm * v);
        scatter(Klap, b, 1, x, y, gm);
        /* ... + G_c(p) / rho */
        *d_rho += -(g[1] * star(Kgx, b, 3, x, y) + g[2] * star(Kgy, b, 3, x, y)) / (rho * rho);
        scatter(Kgx, b, 3, x, y, g[1] / rho);
        scatter(Kgy, b, 3, x, y, g[2] / rho);
    }
    for (int c = 0; c < C; ++c) top[c] = 0.0;
    for (int i = 0; i < N; ++i) top[(i / PLANE) % C] = fmax(top[(i / PLANE) % C], fabs(G[i]));
}

int main(void)
{
    int failures = 0;
    EXPECT(pre_cnsvjp_abi_version() == PRE_CNSVJP_ABI_VERSION, "pre_cnsvjp_abi_version");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    const float s1 = 1.0f / 0.0078f, s2 = 1.0f / (0.0078f * 0.0078f), gamma = 5.0f / 3.0f, scale = 1e-4f;
    /* distinct crosses: a caller's kernels, not the constructor's */
    const float Kgx[9] = {0, -0.5f * s1, 0, 0, 0, 0, 0, 0.5f * s1, 0}, Kgy[9] = {0, 0, 0, -0.25f * s1, 0.125f, 0.75f * s1, 0, 0, 0};
    const float Kdx[9] = {0, -0.5f * s1, 0, 0.5f, 1.0f, 0, 0, 0.5f * s1, 0}, Kdy[9] = {0, 2.0f, 0, -0.5f * s1, 0, 0.5f * s1, 0, -1.0f, 0};
    const float Klap[9] = {0, s2, 0, s2, -4.0f * s2, s2, 0, s2, 0};
    const pre_bc_t bc = {{PRE_BC_PERIODIC, PRE_BC_REPLICATE, PRE_BC_PERIODIC, PRE_BC_REPLICATE}, {0, 0, 0, 0}};
    /* left constant 0 (rho maps to 0 there: 1/rho is inf outside), right reflect, top reflect, bottom periodic */
    const pre_bc_t bc2 = {{PRE_BC_CONSTANT, PRE_BC_REFLECT, PRE_BC_REFLECT, PRE_BC_PERIODIC}, {0, 0, 0, 0}};

    float *hv = malloc(sizeof(float) * N), *hg = malloc(sizeof(float) * N), *ho = malloc(sizeof(float) * N);
    G = malloc(sizeof(double) * N);
    unsigned seed = 11u;
    for (int i = 0; i < N; ++i) hv[i] = frand(&seed);
    for (int i = 0; i < N; ++i) hg[i] = 2.0f * (frand(&seed) - 1.0f);
    H = hv;

    float *dv, *dg, *dout;
    CHECK_HIP(hipMalloc((void **)&dv, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dg, sizeof(float) * N));
    CHECK_HIP(hipMalloc((void **)&dout, sizeof(float) * N));
    CHECK_HIP(hipMemcpy(dv, hv, sizeof(float) * N, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dg, hg, sizeof(float) * N, hipMemcpyHostToDevice));
    pre_cns_plane_t in[4], cot[4], acc[4];
    pre_cns_out_t gin[4];
    for (int c = 0; c < C; ++c) {
        in[c].ptr = dv + c * PLANE; in[c].sB = C * PLANE; in[c].sX = Y;
        cot[c].ptr = dg + c * PLANE; cot[c].sB = C * PLANE; cot[c].sX = Y;
        gin[c].ptr = dout + c * PLANE; gin[c].sB = C * PLANE; gin[c].sX = Y;
        acc[c].ptr = dout + c * PLANE; acc[c].sB = C * PLANE; acc[c].sX = Y;
    }
    double top[4], worst;

    /* ---- the bare product under both boundary mappings */
    XLO = X - 1; XHI = X - 1; YLO = Y - 1; YHI = Y - 1;
    reference(hg, Kgx, Kgy, Kdx, Kdy, Klap, (double)gamma, top);
    CHECK_HIP(hipMemset(dout, 0xff, sizeof(float) * N));
    EXPECT(pre_cns_vjp_f32(in, cot, gin, Kgx, Kgy, Kdx, Kdy, Klap, &bc, gamma, NULL, 0.0f, B, X, Y, 0, NULL) == PRE_OK, "pre_cns_vjp_f32 returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(ho, dout, sizeof(float) * N, hipMemcpyDeviceToHost));
    worst = 0.0;
    for (int i = 0; i < N; ++i) worst = fmax(worst, fabs((double)ho[i] - G[i]) / top[(i / PLANE) % C]);
    printf("      worst channel-scale error: vjp %.3e\n", worst);
    EXPECT(worst <= 1e-5, "vjp matches the scattered product in double within 1e-5 of each channel's scale");

    /* ---- the epilogue: gin = gin + scale * vjp (in place), then gin = cot + scale * vjp */
    EXPECT(pre_cns_vjp_f32(in, cot, gin, Kgx, Kgy, Kdx, Kdy, Klap, &bc, gamma, acc, scale, B, X, Y, 0, NULL) == PRE_OK,
           "pre_cns_vjp_f32 with the epilogue, add_to == gin, returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    float *h2 = malloc(sizeof(float) * N);
    CHECK_HIP(hipMemcpy(h2, dout, sizeof(float) * N, hipMemcpyDeviceToHost));
    worst = 0.0;
    for (int i = 0; i < N; ++i) worst = fmax(worst, fabs((double)h2[i] - (1.0 + (double)scale) * G[i]) / top[(i / PLANE) % C]);
    EXPECT(worst <= 1e-5, "add_to + scale * vjp, in place, matches within 1e-5");
    EXPECT(pre_cns_vjp_f32(in, cot, gin, Kgx, Kgy, Kdx, Kdy, Klap, &bc, gamma, cot, scale, B, X, Y, 0, NULL) == PRE_OK,
           "pre_cns_vjp_f32 with add_to == cot returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(h2, dout, sizeof(float) * N, hipMemcpyDeviceToHost));
    worst = 0.0;
    for (int i = 0; i < N; ++i)
        worst = fmax(worst, fabs((double)h2[i] - ((double)hg[i] + (double)scale * G[i])) / (1.0 + (double)scale * top[(i / PLANE) % C]));
    EXPECT(worst <= 1e-5, "cot + scale * vjp matches within 1e-5");

    XLO = 1; XHI = 0; YLO = -1; YHI = Y - 2;
    VXLO = VXHI = VYLO = VYHI = 0.0;
    reference(hg, Kgx, Kgy, Kdx, Kdy, Klap, (double)gamma, top);
    EXPECT(pre_cns_vjp_f32(in, cot, gin, Kgx, Kgy, Kdx, Kdy, Klap, &bc2, gamma, NULL, 0.0f, B, X, Y, 0, NULL) == PRE_OK,
           "pre_cns_vjp_f32 under constant 0 / reflect / reflect / periodic returns PRE_OK");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(ho, dout, sizeof(float) * N, hipMemcpyDeviceToHost));
    worst = 0.0;
    int finite = 1;
    for (int i = 0; i < N; ++i) {
        finite = finite && isfinite(ho[i]);
        worst = fmax(worst, fabs((double)ho[i] - G[i]) / top[(i / PLANE) % C]);
    }
    printf("      worst channel-scale error under the second mapping: %.3e\n", worst);
    EXPECT(finite, "a constant side of value 0 leaves no NaN (w is masked outside the domain)");
    EXPECT(worst <= 1e-5, "vjp under the second mapping matches within 1e-5");

    /* ---- argument errors: nothing is launched, gin keeps its sentinel */
    CHECK_HIP(hipMemset(dout, 0x55, sizeof(float) * N));
#define CALL(IN, COT, GIN, KGX, BCP, ADD, XX, YY, FL) pre_cns_vjp_f32(IN, COT, GIN, KGX, Kgy, Kdx, Kdy, Klap, BCP, gamma, ADD, scale, B, XX, YY, FL, NULL)
    EXPECT(CALL(NULL, cot, gin, Kgx, &bc, NULL, X, Y, 0) == PRE_E_NULL, "null in -> PRE_E_NULL");
    EXPECT(CALL(in, NULL, gin, Kgx, &bc, NULL, X, Y, 0) == PRE_E_NULL, "null cot -> PRE_E_NULL");
    EXPECT(CALL(in, cot, gin, NULL, &bc, NULL, X, Y, 0) == PRE_E_NULL, "null kernel -> PRE_E_NULL");
    EXPECT(CALL(in, cot, gin, Kgx, NULL, NULL, X, Y, 0) == PRE_E_NULL, "null bc -> PRE_E_NULL");
    EXPECT(CALL(in, cot, gin, Kgx, &bc, NULL, X, 6, 0) == PRE_E_UNSUPPORTED, "Y % 4 != 0 -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(in, cot, gin, Kgx, &bc, NULL, 1, Y, 0) == PRE_E_UNSUPPORTED, "X < 2 -> PRE_E_UNSUPPORTED");
    EXPECT(CALL(in, cot, gin, Kgx, &bc, NULL, X, Y, 1) == PRE_E_UNSUPPORTED, "unknown flag -> PRE_E_UNSUPPORTED");
    pre_cns_plane_t off[4];
    memcpy(off, cot, sizeof off);
    off[1].ptr = cot[1].ptr + 1;
    EXPECT(CALL(in, off, gin, Kgx, &bc, NULL, X, 12, 0) == PRE_E_UNSUPPORTED, "a cotangent plane off by one float -> PRE_E_UNSUPPORTED");
    float Kbad[9];
    memcpy(Kbad, Kgx, sizeof Kbad);
    Kbad[8] = 1.0f;
    EXPECT(CALL(in, cot, gin, Kbad, &bc, NULL, X, Y, 0) == PRE_E_UNSUPPORTED, "a kernel off the cross -> PRE_E_UNSUPPORTED");
    pre_bc_t bad = bc;
    bad.mode[1] = 7;
    EXPECT(CALL(in, cot, gin, Kgx, &bad, NULL, X, Y, 0) == PRE_E_RANGE, "unknown boundary mode -> PRE_E_RANGE");
    pre_cns_out_t onto[4];
    memcpy(onto, gin, sizeof onto);
    onto[0].ptr = dv + 3 * PLANE;
    EXPECT(CALL(in, cot, onto, Kgx, &bc, NULL, X, Y, 0) == PRE_E_RANGE, "gin on in -> PRE_E_RANGE");
    onto[0].ptr = dg + 2 * PLANE;
    EXPECT(CALL(in, cot, onto, Kgx, &bc, NULL, X, Y, 0) == PRE_E_RANGE, "gin on cot -> PRE_E_RANGE");
    pre_cns_plane_t shifted[4];
    memcpy(shifted, acc, sizeof shifted);
    for (int c = 0; c < C; ++c) shifted[c].ptr = dout + c * PLANE + Y;
    EXPECT(CALL(in, cot, gin, Kgx, &bc, shifted, X - 1, Y, 0) == PRE_E_RANGE, "add_to overlapping gin without being it -> PRE_E_RANGE");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(ho, dout, sizeof(float) * N, hipMemcpyDeviceToHost));
    int intact = 1;
    for (size_t i = 0; i < sizeof(float) * N; ++i) intact = intact && ((unsigned char *)ho)[i] == 0x55;
    EXPECT(intact, "no refused call wrote gin");
    hipFree(dv); hipFree(dg); hipFree(dout);
    free(hv); free(hg); free(ho); free(h2); free(G);
    return failures ? 1 : 0;
}
