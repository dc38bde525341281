/* A C99 client of libcp_pre_screenjorekcells.so: a tiny batch of the reduced-MHD fields (rho, phi, T) and the radius R,
 * screened with both equations of pre_residual_jorek_f32 against three per-cell level fields in both layouts - Ny-fastest
 * (memory [B][T][X][Y], pre_screenjorekcells_f32) and Nt-fastest (memory [B][X][Y][T], what Marginal/JOREK_residuals_CP.py
 * holds, pre_screenjorekcells_flat_f32) - checked against plain C loops (the definitions of cp_pre_screenjorekcells.h;
 * Marginal/JOREK_residuals_CP.py:210-243, 297-311) and, when the caller hands them over, against the caller's own values;
 * plus the PRE_E_NULL / PRE_E_RANGE / PRE_E_SHAPE / PRE_E_UNSUPPORTED cases of the header.  Exit code 0 = all ok.
 *
 * Every input is a short closed form of its index, exact in float (LCG(state), the top 16 bits of a 32-bit linear
 * congruential generator as a fraction, see frand), so that the caller can rebuild the inputs bit for bit:
 *   field c (0 rho, 1 phi, 2 T), logical order [B][T][X][Y]:  1 + 0.125 c + 0.25 (frand - 0.5), one stream over c, then i
 *   modulation [T][X][Y]:                                     0.75 + 0.5 frand, the same stream continued
 *   level field k [T][X][Y]:                                  LEVEL[k] * (0.75 + 0.5 frand), the same stream continued
 *   R[y] = 1 + y / (Y - 1);  the operators of the script (Marginal/JOREK_residuals_CP.py:201-205)
 *
 * Arguments (optional): 2 * (B + 2 NK B) numbers - per equation (continuity, then temperature) the B scores, the NK * B
 * counts [k][b] and the NK * B numbers of undecided cells [k][b] of the caller's float64 reference with crop 1 and the
 * modulation; the launches of both layouts are then held to them as well (score within 1e-5 max |r| / min m + 1e-6 of it,
 * the C loops' own bound; a count within the undecided cells).
 *
 *   gcc -std=c99 -D__HIP_PLATFORM_AMD__ tests/c_abi/screenjorekcells_check.c -Iinclude -I/opt/rocm/include -Lcp_pre_amd
 *       -l:libcp_pre_screenjorekcells.so -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/cp_pre_amd -lm -o screenjorekcells_check
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cp_pre_screenjorekcells.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); return 2; } } while (0)
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } else { printf("ok:   %s\n", what); } } while (0)

/* T = 6 and Y = 12: Nt-fastest rows of 6 cells, every other row end inside a quad; Y a multiple of 4 for the Ny-fastest form */
enum { B = 2, T = 6, X = 5, Y = 12, CELLS = T * X * Y, NF = 3, NK = 3, NARG = 2 * (B + 2 * NK * B) };

static float frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 16) / 65536.0f; }
/* host fields are kept in logical order [B][T][X][Y] */
static size_t at(int b, int t, int x, int y) { return (((size_t)b * T + t) * X + x) * Y + y; }
static double cell(const float *f, int b, int t, int x, int y)
{
    return (t >= 0 && t < T && x >= 0 && x < X && y >= 0 && y < Y) ? (double)f[at(b, t, x, y)] : 0.0;
}
/* a dense 3x3x3 kernel on (T, X, Y) applied at one cell, zero padding */
static double op(const float *K, const float *f, int b, int t, int x, int y)
{
    double s = 0.0;
    for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) for (int d = 0; d < 3; ++d)
        if (K[(a * 3 + c) * 3 + d] != 0.0f) s += (double)K[(a * 3 + c) * 3 + d] * cell(f, b, t + a - 1, x + c - 1, y + d - 1);
    return s;
}

static float Kt[27], KR[27], KZ[27], KRR[27], KZZ[27], Rr[Y];
static const float coefc[4] = {1.0f, 1.0f, 2.0f, 3.4f}, coeft[4] = {10.0f / 3.0f, 0.0f, 0.0f, 2.25e-7f};
static const float LEVEL[NK] = {0.25f, 1.0f, 1048576.0f};

/* equation `eq` of pre_residual_jorek_f32 at one cell, in double (star_march.h states the expressions) */
static double residual(int eq, float *const *f, int b, int t, int x, int y)
{
    const float *rho = f[0], *phi = f[1], *Tm = f[2];
    const double R = (double)Rr[y], rc = cell(rho, b, t, x, y), tc = cell(Tm, b, t, x, y);
    const double dZphi = op(KZ, phi, b, t, x, y), dRphi = op(KR, phi, b, t, x, y);
    const double Xr = op(KR, rho, b, t, x, y) * dZphi - dRphi * op(KZ, rho, b, t, x, y);
    if (eq == 0) {
        const double Yr = op(KRR, rho, b, t, x, y) + (1.0 / R) * op(KR, rho, b, t, x, y) + op(KZZ, rho, b, t, x, y);
        return (double)coefc[0] * op(Kt, rho, b, t, x, y) - (double)coefc[1] * R * Xr - (double)coefc[2] * rc * dZphi - (double)coefc[3] * Yr;
    }
    {
        const double XT = op(KR, Tm, b, t, x, y) * dZphi - dRphi * op(KZ, Tm, b, t, x, y);
        const double YT = op(KRR, Tm, b, t, x, y) + (1.0 / R) * op(KR, Tm, b, t, x, y) + op(KZZ, Tm, b, t, x, y);
        return tc * op(Kt, rho, b, t, x, y) + rc * op(Kt, Tm, b, t, x, y) - rc * R * XT + tc * R * Xr +
               (double)coeft[0] * rc * tc * dZphi + (double)coeft[3] * YT;
    }
}

/* compare the accumulators `acc` ([NK + 1][B]) with the loops over t in [1, T-1), x in [1, X-1), y in [1, Y-1); hm the
 * modulation and hl the NK level fields in logical order [T][X][Y]; want: the caller's values of this equation, or NULL */
static int matches(int eq, float *const *hf, const float *hm, const float *hl, const uint32_t *acc, const double *want, const char *name)
{
    double rmax = 0.0, mmin = 1e30;
    int ok = 1;
    for (int pass = 0; pass < 2 && ok; ++pass)
        for (int b = 0; b < B; ++b) {
            double want_s = 0.0;
            long want_c[NK] = {0, 0, 0}, und[NK] = {0, 0, 0};
            for (int t = 1; t < T - 1; ++t) for (int x = 1; x < X - 1; ++x) for (int y = 1; y < Y - 1; ++y) {
                const size_t i = ((size_t)t * X + x) * Y + y;
                const double r = fabs(residual(eq, hf, b, t, x, y)), m = hm[i];
                if (pass == 0) { rmax = fmax(rmax, r); mmin = fmin(mmin, m); continue; }
                want_s = fmax(want_s, r / m);
                for (int k = 0; k < NK; ++k) {
                    const double hw = (double)hl[(size_t)k * CELLS + i] * m;
                    if (r <= hw) ++want_c[k];
                    if (fabs(r - hw) <= 1e-5 * rmax) ++und[k];
                }
            }
            if (pass == 0) continue;
            float got;
            memcpy(&got, &acc[b], sizeof(float));
            printf("      %s sample %d: score %.7g (C loop %.7g), counts %u %u %u (C loop %ld %ld %ld)\n", name, b, got, want_s,
                   acc[B + b], acc[2 * B + b], acc[3 * B + b], want_c[0], want_c[1], want_c[2]);
            if (!(fabs(got - want_s) <= 1e-5 * rmax / mmin + 1e-6 * want_s)) ok = 0;
            for (int k = 0; k < NK; ++k)
                if (labs((long)acc[(1 + k) * B + b] - want_c[k]) > und[k]) ok = 0;
            if (acc[3 * B + b] != (T - 2) * (X - 2) * (Y - 2)) ok = 0;      /* a level above every score holds every counted cell */
            if (want) {                                                      /* the caller's float64 reference */
                printf("      %s sample %d: the caller's score %.7g, counts %.0f %.0f %.0f (undecided %.0f %.0f %.0f)\n", name, b,
                       want[b], want[B + b], want[B + B + b], want[B + 2 * B + b], want[B + NK * B + b],
                       want[B + NK * B + B + b], want[B + NK * B + 2 * B + b]);
                if (!(fabs(got - want[b]) <= 1e-5 * rmax / mmin + 1e-6 * want[b])) ok = 0;
                for (int k = 0; k < NK; ++k)
                    if (fabs((double)acc[(1 + k) * B + b] - want[B + k * B + b]) > want[B + NK * B + k * B + b]) ok = 0;
            }
        }
    return ok;
}

int main(int argc, char **argv)
{
    int failures = 0;
    EXPECT(pre_screenjorekcells_abi_version() == PRE_SCREENJOREKCELLS_ABI_VERSION, "pre_screenjorekcells_abi_version");
    EXPECT(pre_screenjorekcells_sample_group() >= 1, "pre_screenjorekcells_sample_group");
    double given[NARG];
    const int have = argc == 1 + NARG;
    if (argc != 1 && !have) { printf("FAIL: %d arguments, expected none or %d\n", argc - 1, (int)NARG); return 1; }
    for (int i = 0; i < NARG && have; ++i) given[i] = strtod(argv[1 + i], NULL);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no device: ABI checks only\n");
        return failures ? 1 : 0;
    }
    /* operators on (T, X, Y): index (a * 3 + c) * 3 + d = offset (a - 1, c - 1, d - 1); D_Z and D_ZZ with their taps along T,
     * as the script's 'y' operators have them */
    Kt[(0 * 3 + 1) * 3 + 1] = -1.0f; Kt[(2 * 3 + 1) * 3 + 1] = 1.0f;
    KR[(1 * 3 + 0) * 3 + 1] = -1.0f; KR[(1 * 3 + 2) * 3 + 1] = 1.0f;
    KZ[(0 * 3 + 1) * 3 + 1] = -1.0f; KZ[(2 * 3 + 1) * 3 + 1] = 1.0f;
    KRR[13] = -2.0f * (5.0f / 3.0f); KRR[(1 * 3 + 0) * 3 + 1] = KRR[(1 * 3 + 2) * 3 + 1] = 5.0f / 3.0f;
    KZZ[13] = -2.0f * (5.0f / 3.0f); KZZ[(0 * 3 + 1) * 3 + 1] = KZZ[(2 * 3 + 1) * 3 + 1] = 5.0f / 3.0f;
    for (int y = 0; y < Y; ++y) Rr[y] = 1.0f + (float)y / (float)(Y - 1);

    float *hf[NF], *hm = malloc(sizeof(float) * CELLS), *hl = malloc(sizeof(float) * NK * CELLS);
    float *tmp = malloc(sizeof(float) * (B > NK ? B : NK) * CELLS);
    unsigned s = 5u;
    for (int c = 0; c < NF; ++c) {
        hf[c] = malloc(sizeof(float) * B * CELLS);
        for (int i = 0; i < B * CELLS; ++i) hf[c][i] = 1.0f + 0.125f * (float)c + 0.25f * (frand(&s) - 0.5f);
    }
    for (int i = 0; i < CELLS; ++i) hm[i] = 0.75f + 0.5f * frand(&s);
    for (int k = 0; k < NK; ++k) for (int i = 0; i < CELLS; ++i) hl[(size_t)k * CELLS + i] = LEVEL[k] * (0.75f + 0.5f * frand(&s));

    /* device: per layout NF fields, the modulation, the level fields and the R view; [0] Ny-fastest, [1] Nt-fastest */
    float *df[2], *dm[2], *dl[2], *dR[2];
    uint32_t *dacc;
    for (int l = 0; l < 2; ++l) {
        CHECK_HIP(hipMalloc((void **)&df[l], sizeof(float) * NF * B * CELLS));
        CHECK_HIP(hipMalloc((void **)&dm[l], sizeof(float) * CELLS));
        CHECK_HIP(hipMalloc((void **)&dl[l], sizeof(float) * NK * CELLS));
        CHECK_HIP(hipMalloc((void **)&dR[l], sizeof(float) * Y * T));
    }
    CHECK_HIP(hipMalloc((void **)&dacc, sizeof(uint32_t) * (NK + 1) * B));
    for (int c = 0; c < NF; ++c) {
        CHECK_HIP(hipMemcpy(df[0] + (size_t)c * B * CELLS, hf[c], sizeof(float) * B * CELLS, hipMemcpyHostToDevice));
        for (int b = 0; b < B; ++b) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y)
            tmp[(((size_t)b * X + x) * Y + y) * T + t] = hf[c][at(b, t, x, y)];
        CHECK_HIP(hipMemcpy(df[1] + (size_t)c * B * CELLS, tmp, sizeof(float) * B * CELLS, hipMemcpyHostToDevice));
    }
    CHECK_HIP(hipMemcpy(dm[0], hm, sizeof(float) * CELLS, hipMemcpyHostToDevice));
    for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y)
        tmp[((size_t)x * Y + y) * T + t] = hm[((size_t)t * X + x) * Y + y];
    CHECK_HIP(hipMemcpy(dm[1], tmp, sizeof(float) * CELLS, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dl[0], hl, sizeof(float) * NK * CELLS, hipMemcpyHostToDevice));
    for (int k = 0; k < NK; ++k) for (int t = 0; t < T; ++t) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y)
        tmp[(size_t)k * CELLS + ((size_t)x * Y + y) * T + t] = hl[(size_t)k * CELLS + ((size_t)t * X + x) * Y + y];
    CHECK_HIP(hipMemcpy(dl[1], tmp, sizeof(float) * NK * CELLS, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dR[0], Rr, sizeof(float) * Y, hipMemcpyHostToDevice));
    for (int y = 0; y < Y; ++y) for (int t = 0; t < T; ++t) tmp[y * T + t] = Rr[y];
    CHECK_HIP(hipMemcpy(dR[1], tmp, sizeof(float) * Y * T, hipMemcpyHostToDevice));

    pre_field_t fy[NF], ft[NF];
    for (int c = 0; c < NF; ++c) {
        const pre_field_t a = {df[0] + (size_t)c * B * CELLS, (int64_t)CELLS, (int64_t)X * Y, Y, 1};     /* sB, sT, sX, sY */
        const pre_field_t v = {df[1] + (size_t)c * B * CELLS, (int64_t)CELLS, 1, (int64_t)Y * T, T};
        fy[c] = a; ft[c] = v;
    }
    const pre_field_t Ry = {dR[0], 0, 0, 0, 1}, Rt = {dR[1], 0, 1, 0, T};
    /* levels, nk, lK, lT, lX (, lY), modulation, mT, mX (, mY), ct, cx, cy, score, count, count_ld */
    const pre_screencells_t sy = {dl[0], NK, (int64_t)CELLS, (int64_t)X * Y, Y, dm[0], (int64_t)X * Y, Y, 1, 1, 1, dacc, dacc + B, B};
    const pre_screencellsflat_t st = {dl[1], NK, (int64_t)CELLS, 1, (int64_t)Y * T, T, dm[1], 1, (int64_t)Y * T, T, 1, 1, 1, dacc,
                                      dacc + B, B};
    uint32_t acc[(NK + 1) * B], again[(NK + 1) * B], flat[(NK + 1) * B];
    int rc;

    /* ---- both equations in both layouts against the loops (and the caller's values) */
    for (int eq = 0; eq < 2; ++eq) {
        const float *coef = eq == 0 ? coefc : coeft;
        const double *want = have ? given + eq * (NARG / 2) : NULL;
        CHECK_HIP(hipMemset(dacc, 0, sizeof(acc)));
        rc = pre_screenjorekcells_f32(eq, fy, &Ry, Kt, KR, KZ, KRR, KZZ, coef, &sy, B, T, X, Y, 0, NULL);
        EXPECT(rc == PRE_OK, eq == 0 ? "pre_screenjorekcells_f32 (continuity) returns PRE_OK" : "pre_screenjorekcells_f32 (temperature) returns PRE_OK");
        CHECK_HIP(hipDeviceSynchronize());
        CHECK_HIP(hipMemcpy(acc, dacc, sizeof(acc), hipMemcpyDeviceToHost));
        EXPECT(matches(eq, hf, hm, hl, acc, want, "Ny-fastest"), "Ny-fastest: scores and counts match the C loops (crop, modulation, level fields)");

        CHECK_HIP(hipMemset(dacc, 0, sizeof(acc)));
        rc = pre_screenjorekcells_flat_f32(eq, ft, &Rt, Kt, KR, KZ, KRR, KZZ, coef, &st, B, T, X, Y, 0, NULL);
        EXPECT(rc == PRE_OK, eq == 0 ? "pre_screenjorekcells_flat_f32 (continuity) returns PRE_OK" : "pre_screenjorekcells_flat_f32 (temperature) returns PRE_OK");
        CHECK_HIP(hipDeviceSynchronize());
        CHECK_HIP(hipMemcpy(flat, dacc, sizeof(flat), hipMemcpyDeviceToHost));
        EXPECT(matches(eq, hf, hm, hl, flat, want, "Nt-fastest"), "Nt-fastest: scores and counts match the C loops (crop, modulation, level fields)");

        /* the same call again without zeroing: the counts double, the score stays */
        rc = pre_screenjorekcells_flat_f32(eq, ft, &Rt, Kt, KR, KZ, KRR, KZZ, coef, &st, B, T, X, Y, 0, NULL);
        EXPECT(rc == PRE_OK, "second call into the same buffers");
        CHECK_HIP(hipDeviceSynchronize());
        CHECK_HIP(hipMemcpy(again, dacc, sizeof(again), hipMemcpyDeviceToHost));
        {
            int ok = memcmp(flat, again, sizeof(uint32_t) * B) == 0;
            for (int i = B; i < (NK + 1) * B; ++i) ok = ok && again[i] == 2 * flat[i];
            EXPECT(ok, "two calls: counts doubled, score kept");
        }
    }
    CHECK_HIP(hipMemcpy(acc, dacc, sizeof(acc), hipMemcpyDeviceToHost));

    /* ---- the cases of the header that are refused before any launch */
    EXPECT(pre_screenjorekcells_f32(0, NULL, &Ry, Kt, KR, KZ, KRR, KZZ, coefc, &sy, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null fields -> PRE_E_NULL");
    EXPECT(pre_screenjorekcells_f32(0, fy, NULL, Kt, KR, KZ, KRR, KZZ, coefc, &sy, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null R -> PRE_E_NULL");
    EXPECT(pre_screenjorekcells_f32(0, fy, &Ry, Kt, KR, KZ, KRR, NULL, coefc, &sy, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null kernel -> PRE_E_NULL");
    EXPECT(pre_screenjorekcells_f32(0, fy, &Ry, Kt, KR, KZ, KRR, KZZ, NULL, &sy, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null coef -> PRE_E_NULL");
    EXPECT(pre_screenjorekcells_f32(0, fy, &Ry, Kt, KR, KZ, KRR, KZZ, coefc, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null pre_screencells_t -> PRE_E_NULL");
    EXPECT(pre_screenjorekcells_flat_f32(1, ft, NULL, Kt, KR, KZ, KRR, KZZ, coeft, &st, B, T, X, Y, 0, NULL) == PRE_E_NULL, "flat: null R -> PRE_E_NULL");
    EXPECT(pre_screenjorekcells_flat_f32(1, ft, &Rt, Kt, KR, KZ, KRR, KZZ, coeft, NULL, B, T, X, Y, 0, NULL) == PRE_E_NULL, "flat: null pre_screencellsflat_t -> PRE_E_NULL");
    pre_screencells_t bad = sy;
    bad.levels = NULL;
    EXPECT(pre_screenjorekcells_f32(0, fy, &Ry, Kt, KR, KZ, KRR, KZZ, coefc, &bad, B, T, X, Y, 0, NULL) == PRE_E_NULL, "null level fields -> PRE_E_NULL");
    EXPECT(pre_screenjorekcells_f32(2, fy, &Ry, Kt, KR, KZ, KRR, KZZ, coefc, &sy, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "eq 2 -> PRE_E_RANGE");
    EXPECT(pre_screenjorekcells_flat_f32(-1, ft, &Rt, Kt, KR, KZ, KRR, KZZ, coefc, &st, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "flat: eq -1 -> PRE_E_RANGE");
    bad = sy;
    bad.nk = 17;
    EXPECT(pre_screenjorekcells_f32(0, fy, &Ry, Kt, KR, KZ, KRR, KZZ, coefc, &bad, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "17 levels -> PRE_E_RANGE");
    bad = sy;
    bad.ct = -1;
    EXPECT(pre_screenjorekcells_f32(0, fy, &Ry, Kt, KR, KZ, KRR, KZZ, coefc, &bad, B, T, X, Y, 0, NULL) == PRE_E_RANGE, "negative crop -> PRE_E_RANGE");
    bad = sy;
    bad.lT = -1;
    EXPECT(pre_screenjorekcells_f32(0, fy, &Ry, Kt, KR, KZ, KRR, KZZ, coefc, &bad, B, T, X, Y, 0, NULL) == PRE_E_SHAPE, "negative level stride -> PRE_E_SHAPE");
    pre_screencellsflat_t badf = st;
    badf.lK = -1;
    EXPECT(pre_screenjorekcells_flat_f32(1, ft, &Rt, Kt, KR, KZ, KRR, KZZ, coeft, &badf, B, T, X, Y, 0, NULL) == PRE_E_SHAPE, "flat: negative level stride -> PRE_E_SHAPE");
    badf = st;
    badf.lT = (int64_t)X * Y; badf.lX = Y; badf.lY = 1;
    EXPECT(pre_screenjorekcells_flat_f32(1, ft, &Rt, Kt, KR, KZ, KRR, KZZ, coeft, &badf, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "flat: Ny-fastest level fields -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenjorekcells_f32(0, ft, &Ry, Kt, KR, KZ, KRR, KZZ, coefc, &sy, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "Nt-fastest fields in the Ny-fastest form -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenjorekcells_f32(1, fy, &Rt, Kt, KR, KZ, KRR, KZZ, coeft, &sy, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "R without unit stride on Y -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenjorekcells_f32(0, fy, &Ry, Kt, KR, KZ, KRR, KZZ, coefc, &sy, B, T, X, Y - 2, 0, NULL) == PRE_E_UNSUPPORTED, "Y % 4 != 0 -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenjorekcells_flat_f32(0, fy, &Rt, Kt, KR, KZ, KRR, KZZ, coefc, &st, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "Ny-fastest fields in the flat form -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenjorekcells_flat_f32(0, ft, &Ry, Kt, KR, KZ, KRR, KZZ, coefc, &st, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "flat: R with sT != 1 -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenjorekcells_flat_f32(0, ft, &Rt, Kt, KR, KZ, KRR, KZZ, coefc, &st, B, T, X, Y, PRE_FLAG_HALO_X, NULL) == PRE_E_UNSUPPORTED, "flat: PRE_FLAG_HALO_X -> PRE_E_UNSUPPORTED");
    float Kbox[27] = {0};
    Kbox[0] = 1.0f;
    EXPECT(pre_screenjorekcells_f32(0, fy, &Ry, Kt, Kbox, KZ, KRR, KZZ, coefc, &sy, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "kernel off the star -> PRE_E_UNSUPPORTED");
    EXPECT(pre_screenjorekcells_flat_f32(1, ft, &Rt, Kt, KR, KZ, KRR, Kbox, coeft, &st, B, T, X, Y, 0, NULL) == PRE_E_UNSUPPORTED, "flat: kernel off the star -> PRE_E_UNSUPPORTED");
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(again, dacc, sizeof(again), hipMemcpyDeviceToHost));
    EXPECT(memcmp(acc, again, sizeof(acc)) == 0, "refused calls changed nothing");

    for (int l = 0; l < 2; ++l) { hipFree(df[l]); hipFree(dm[l]); hipFree(dl[l]); hipFree(dR[l]); }
    hipFree(dacc);
    for (int c = 0; c < NF; ++c) free(hf[c]);
    free(hm); free(hl); free(tmp);
    return failures ? 1 : 0;
}
