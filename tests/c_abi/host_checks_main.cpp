// host_checks_main.cpp - the host-side checks of cp_pre_amd/csrc/host_checks.h on the CPU.  tests/test_host_checks_cpu.py
// builds this file with the host compiler under -fsanitize=address,undefined -fno-sanitize-recover=all and runs it: a
// wrong answer exits 1, undefined behaviour or a bad access aborts.  Nothing here is dereferenced on a device; the
// addresses are numbers.
#include <stdio.h>
#include <limits.h>

#include "../../cp_pre_amd/csrc/host_checks.h"

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static const void *at(uintptr_t a) { return (const void *)a; }

// the span of view (base, s, n, halo), which must exist
static Span span(uintptr_t base, const int64_t (&s)[4], const int64_t (&n)[4], int64_t halo = 0)
{
    Span r{1, 0};
    CHECK(span_of(at(base), s, n, halo, &r));
    return r;
}
static bool refused(uintptr_t base, const int64_t (&s)[4], const int64_t (&n)[4], int64_t halo = 0)
{
    Span r;
    return !span_of(at(base), s, n, halo, &r);
}

static void test_span_of()
{
    const uintptr_t base = 0x10000000u;
    const int64_t n[4] = {2, 3, 4, 5}, one[4] = {1, 1, 1, 1};
    const int64_t dense[4] = {60, 20, 5, 1}, back[4] = {-60, 20, 5, 1}, zero[4] = {0, 0, 0, 1}, wide[4] = {7, 7, 7, 4};
    const int64_t big = (int64_t)1 << 62;
    Span s = span(base, dense, n);                                  // positive strides: 120 floats from the base
    CHECK(s.lo == base && s.hi == base + 480);
    s = span(base, back, n);                                        // a negative stride: 60 floats below, 60 from the base
    CHECK(s.lo == base - 240 && s.hi == base + 240);
    s = span(base, zero, wide);                                     // zero strides: one row of 4 floats, whatever the extents
    CHECK(s.lo == base && s.hi == base + 16);
    s = span(base, dense, n, 5);                                    // the halo stride: one row more on either side
    CHECK(s.lo == base - 20 && s.hi == base + 500);
    s = span(base, dense, n, -5);                                   // ... of either sign
    CHECK(s.lo == base - 20 && s.hi == base + 500);
    const int64_t huge[4] = {big, -big, big, LLONG_MAX};
    s = span(base, huge, one);                                      // extent 1: a stride is never applied
    CHECK(s.lo == base && s.hi == base + 4);

    // two views that touch are disjoint; two that share one float are not
    const Span a = span(base, dense, n);
    CHECK(!overlaps(a, span(base + 480, dense, n)) && !overlaps(span(base + 480, dense, n), a));
    CHECK(overlaps(a, span(base + 476, dense, n)) && overlaps(span(base + 476, dense, n), a));
    CHECK(!overlaps(a, span(base - 480, dense, n)) && overlaps(a, span(base - 476, dense, n)));
    CHECK(overlaps(a, a));

    // offsets that leave int64: a product, a sum, the bytes of a sum that fits in elements, the halo
    const int64_t n4[4] = {4, 1, 1, 1}, n22[4] = {2, 2, 1, 1};
    const int64_t p[4] = {big, 1, 1, 1}, q[4] = {big, big, 1, 1}, m[4] = {-big, -big, 1, 1}, r[4] = {big / 2, 1, 1, 1};
    CHECK(refused(base, p, n4));                                    // 2^62 * 3
    CHECK(refused(base, q, n22));                                   // 2^62 + 2^62
    CHECK(refused(base, m, n22));                                   // -2^63 elements below: the bytes leave int64
    CHECK(refused(base, r, n22));                                   // 2^61 elements are 2^63 bytes
    CHECK(refused(base, dense, n, LLONG_MIN) && refused(base, dense, n, LLONG_MAX));
    const int64_t sb62[4] = {big, 128, 16, 1}, nb[4] = {2, 1, 8, 16};
    CHECK(refused(base, sb62, nb));                                 // the probe of the CPU refusal tests: sb = 2^62, B = 2

    // the ends of the address space: a span may end below 2^64 and start at 0, not beyond either
    const int64_t row[4] = {0, 0, 0, 1}, f4[4] = {1, 1, 1, 4}, f8[4] = {1, 1, 1, 8}, down[4] = {-4, 0, 0, 1}, two[4] = {2, 1, 1, 4};
    const uintptr_t top = UINTPTR_MAX - 31;                         // 32 bytes below the top
    s = span(top, row, f4);
    CHECK(s.lo == top && s.hi == top + 16 && s.lo < s.hi);
    CHECK(refused(top, row, f8));                                   // would end at 2^64
    CHECK(refused(top + 16, row, f4));                              // hi would be 2^64 itself
    s = span(16, down, two);                                        // 4 floats below address 16: starts at 0
    CHECK(s.lo == 0 && s.hi == 32);
    CHECK(refused(12, down, two));                                  // would start below 0
    CHECK(!overlaps(span(top, row, f4), span(16, down, two)));
}

static void test_plane_and_alignment()
{
    // (X - 1) * sX + Y must stay inside int32: e > -(2^31 - 1) and e < 2^31 - 1 - Y
    CHECK(plane_fits_int32(1, 0x7fffffffLL - 16, 16));              // e = 2^31 - 18
    CHECK(!plane_fits_int32(1, 0x7fffffffLL - 15, 16));             // e = 2^31 - 17 = 2^31 - 1 - Y
    CHECK(plane_fits_int32(-1, 0x7fffffffLL, 16));                  // e = -(2^31 - 2)
    CHECK(!plane_fits_int32(-1, 0x80000000LL, 16));                 // e = -(2^31 - 1)
    CHECK(plane_fits_int32(0, LLONG_MAX, 4) && plane_fits_int32(16, 8, 16));
    CHECK(!plane_fits_int32((int64_t)1 << 30, 8, 16) && !plane_fits_int32((int64_t)1 << 62, 8, 16));     // the product leaves int64

    CHECK(aligned16(at(0x1000), 128, 16, 2));
    CHECK(!aligned16(at(0x1004), 128, 16, 2) && !aligned16(at(0x1008), 128, 16, 2));
    CHECK(!aligned16(at(0x1000), 128, 18, 2) && aligned16(at(0x1000), 128, -16, 2) && aligned16(at(0x1000), 128, 0, 2));
    CHECK(!aligned16(at(0x1000), 130, 16, 2) && aligned16(at(0x1000), 130, 16, 1));      // the batch stride of one sample is not used
}

static void test_boundaries()
{
    int idx;
    float val;
    for (int hi = 0; hi < 2; ++hi) {
        idx = 99; val = 99.f;
        CHECK(bc_side(PRE_BC_CONSTANT, 2.5f, 8, hi, &idx, &val) && idx == -1 && val == 2.5f);
        CHECK(bc_side(PRE_BC_REPLICATE, 2.5f, 8, hi, &idx, &val) && idx == (hi ? 7 : 0) && val == 0.f);
        CHECK(bc_side(PRE_BC_PERIODIC, 2.5f, 8, hi, &idx, &val) && idx == (hi ? 0 : 7) && val == 0.f);
        CHECK(bc_side(PRE_BC_REFLECT, 2.5f, 8, hi, &idx, &val) && idx == (hi ? 6 : 1) && val == 0.f);
        CHECK(bc_side(PRE_BC_REFLECT, 2.5f, 2, hi, &idx, &val) && idx == (hi ? 0 : 1));
        CHECK(!bc_side(PRE_BC_REFLECT, 2.5f, 1, hi, &idx, &val));   // nothing to reflect on
        CHECK(bc_side(PRE_BC_REPLICATE, 0.f, 1, hi, &idx, &val) && idx == 0);
        CHECK(bc_side(PRE_BC_PERIODIC, 0.f, 1, hi, &idx, &val) && idx == 0);
        CHECK(!bc_side(4, 0.f, 8, hi, &idx, &val) && !bc_side(-1, 0.f, 8, hi, &idx, &val));
    }
    // pre_bc_t: left, right (columns, Y), top, bottom (rows, X)
    pre_bc_t bc = {{PRE_BC_PERIODIC, PRE_BC_REPLICATE, PRE_BC_CONSTANT, PRE_BC_REFLECT}, {0.f, 0.f, 1.5f, 0.f}};
    BCInfo o;
    CHECK(bc_info(&bc, 8, 16, &o) && o.ylo == 15 && o.yhi == 15 && o.xlo == -1 && o.vxlo == 1.5f && o.xhi == 6);
    CHECK(!bc_info(&bc, 1, 16, &o));
    bc.mode[0] = 9;
    CHECK(!bc_info(&bc, 8, 16, &o));

    const float plus[9] = {0, 1, 0, 2, 3, 4, 0, 5, 0};
    Cross k;
    CHECK(cross_from_dense9(plus, &k) && k.c == 3 && k.xm == 1 && k.xp == 5 && k.ym == 2 && k.yp == 4);
    const int corners[4] = {0, 2, 6, 8};
    for (int corner : corners) {
        float off[9] = {0, 1, 0, 2, 3, 4, 0, 5, 0};
        off[corner] = 1e-30f;
        CHECK(!cross_from_dense9(off, &k));
    }
}

// the chunk rule of the flat form as the three launchers stated it before they shared flat_chunk, in numbers
static int chunk_rule(long long quads, int Ty, bool staged)
{
    const int halo = staged ? 2 * ((Ty + 3) / 4 < 32 ? (Ty + 3) / 4 : 32) : 0;
    int nt = 512;
    for (int c = nt - 64; c >= 256; c -= 64)
        if ((quads + c - 1) / c * (c + halo) * 100 < (quads + nt - 1) / nt * (nt + halo) * (100 - 8)) nt = c;
    return nt;
}

static void test_flat_chunk()
{
    long long differ = 0;
    for (int staged = 0; staged < 2; ++staged)
        for (int Ty = 1; Ty <= 95; ++Ty)
            for (long long quads = 1; quads <= 4096; ++quads)
                differ += flat_chunk(quads, Ty, staged != 0) != chunk_rule(quads, Ty, staged != 0);
    CHECK(differ == 0);
    CHECK(flat_chunk(640, 10, true) == 320 && flat_chunk(512, 20, true) == 512 && flat_chunk(1280, 20, false) == 448);
}

struct Levels { const float *q; unsigned *score, *count; int nk, ct, cx, cy; long long count_ld; };

static void test_screen_args()
{
    const float q[1] = {0.f};
    unsigned sc[1], cn[1];
    const pre_field_t f = {q, 0, 0, 0, 1};
    const pre_field_t *fs[1] = {&f}, *none[1] = {nullptr};
    Levels s = {q, sc, cn, 3, 0, 1, 2, 4};
    CHECK(screen_args(fs, 1, &s, 16, 4, 5, 6, 8, 8) == PRE_OK);
    CHECK(screen_args(fs, 1, (const Levels *)nullptr, 16, 4, 5, 6, 8, 8) == PRE_E_NULL);
    CHECK(screen_args(none, 1, &s, 16, 4, 5, 6, 8, 8) == PRE_E_NULL && screen_args(fs, 1, &s, 16, 4, 0, 6, 8, 8) == PRE_E_NULL);
    CHECK(screen_args(fs, 1, &s, 2, 4, 5, 6, 8, 8) == PRE_E_RANGE);                     // more levels than the library counts
    CHECK(screen_args(fs, 1, &s, 16, 5, 5, 6, 8, 8) == PRE_E_NULL);                     // count_ld < B
    CHECK(screen_args(fs, 1, &s, 16, 4, 5, 6, 0x7fffffffLL - 7, 8) == PRE_E_SHAPE);
    CHECK(screen_args(fs, 1, &s, 16, 4, 1, 1, 0x7fffffffLL - 7, 0) == PRE_OK);
    CHECK(screen_args(fs, 1, &s, 16, 4, 1 << 11, 1 << 11, 1 << 10, 0) == PRE_E_SHAPE);  // 2^32 cells: the counts are 32-bit
    s.cy = -1;
    CHECK(screen_args(fs, 1, &s, 16, 5, 5, 6, 8, 8) == PRE_E_RANGE);                    // (decided before count_ld)
}

int main()
{
    test_span_of();
    test_plane_and_alignment();
    test_boundaries();
    test_flat_chunk();
    test_screen_args();
    if (failures) {
        printf("%d check(s) failed\n", failures);
        return 1;
    }
    printf("host checks ok\n");
    return 0;
}
