// march_store_checks_main.cpp - plane_offsets_fit_u32 of cp_pre_amd/csrc/host_checks.h on the CPU: the check that decides
// whether a thread's place in a plane may be a 32-bit byte offset into a buffer descriptor.  The marched kernels ask it of
// every input view (a view that fails is PRE_E_UNSUPPORTED) and, in the MARCH_ST_SC1 build, of the output view (a view that
// fails keeps the plain store through a 64-bit pointer: never an error).  tests/test_march_store_checks_cpu.py builds this
// file with the host compiler under -fsanitize=address,undefined -fno-sanitize-recover=all and runs it: a wrong answer
// exits 1, undefined behaviour aborts.  Nothing is allocated: the strides are numbers.
#include <stdio.h>
#include <limits.h>
#include <initializer_list>

#include "../../cp_pre_amd/csrc/host_checks.h"

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

// the rule as launch_tiled stated it before the helper: the largest offset a lane may form, in bytes, stays below 2^32
static bool rule(int64_t sX, int64_t rows, int64_t Y)
{
    return sX >= 0 && (unsigned __int128)rows * (unsigned __int128)sX + (unsigned __int128)Y + 8 < ((unsigned __int128)1 << 30);
}

int main()
{
    const int64_t lim = (int64_t)1 << 30;              // floats in 2^32 bytes
    // an output view [.., X = 127 rows, Y = 512] on tiles of 8 rows: rows = X + NR = 135
    const int64_t X = 127, NR = 8, Y = 512, rows = X + NR;
    // the widest row stride that fits, and the next one: both sides of 2^32
    const int64_t fit = (lim - 8 - Y - 1) / rows;
    CHECK(rows * fit + Y + 8 < lim && rows * (fit + 1) + Y + 8 >= lim);
    CHECK(plane_offsets_fit_u32(fit, rows, Y));
    CHECK(!plane_offsets_fit_u32(fit + 1, rows, Y));
    // exactly at the limit: (rows * sX + Y + 8) * 4 == 2^32 does not fit, one float less does
    const int64_t r2 = 1 << 10, s2 = 1 << 20;          // rows * sX == 2^30
    CHECK(!plane_offsets_fit_u32(s2, r2, 0));
    CHECK(!plane_offsets_fit_u32(s2, r2 - 1, s2 - 8));               // == 2^30
    CHECK(plane_offsets_fit_u32(s2, r2 - 1, s2 - 9));                // == 2^30 - 1
    // what the kernels see every day
    CHECK(plane_offsets_fit_u32(512, 130 + 2 + 8, 512));             // the benchmark's x-slab
    CHECK(plane_offsets_fit_u32(512 + 64, 19 + 8, 520));             // pitched rows
    CHECK(plane_offsets_fit_u32(0, 1000000, 4));                     // a broadcast row (JOREK's radius)
    CHECK(plane_offsets_fit_u32(1, 1, 1));
    // a negative stride has no unsigned offset; neither have negative extents
    CHECK(!plane_offsets_fit_u32(-1, rows, Y));
    CHECK(!plane_offsets_fit_u32(512, -1, Y));
    CHECK(!plane_offsets_fit_u32(512, rows, -1));
    // products and sums that leave int64 are refused, not wrapped
    CHECK(!plane_offsets_fit_u32(LLONG_MAX, 2, 4));
    CHECK(!plane_offsets_fit_u32(LLONG_MAX, 1, 4));
    CHECK(!plane_offsets_fit_u32((int64_t)1 << 62, (int64_t)1 << 2, 4));       // wraps to 0 in 64 bits
    CHECK(!plane_offsets_fit_u32(1, 1, LLONG_MAX));
    // against the rule over a sweep around the limit and over small values
    for (int64_t sX : {(int64_t)0, (int64_t)1, (int64_t)515, fit - 1, fit, fit + 1, lim / 8, lim, lim * 4})
        for (int64_t r : {(int64_t)1, (int64_t)8, (int64_t)27, rows, (int64_t)1 << 20, (int64_t)1 << 31})
            for (int64_t y : {(int64_t)1, (int64_t)4, Y, lim - 9, lim - 8, lim})
                CHECK(plane_offsets_fit_u32(sX, r, y) == rule(sX, r, y));
    if (failures) return 1;
    printf("march store checks ok\n");
    return 0;
}
