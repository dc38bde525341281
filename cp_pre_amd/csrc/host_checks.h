// host_checks.h - the checks an entry point makes of its arguments before anything is launched, stated once for every
// library here.  Plain C++17 and no HIP include: a host compiler builds it alone (tests/c_abi/host_checks_main.cpp runs it
// under the address and undefined-behaviour sanitizers).  The helpers answer yes or no; an entry point maps the answer to
// the code its own header documents.
#pragma once
#include <stdint.h>
#include "../../include/cp_pre_hip.h"

namespace {

// ---- the bytes a strided view addresses ------------------------------------------------------------------------------
struct Span { uintptr_t lo, hi; };                 // byte addresses [lo, hi)

// The span of a 4-D strided fp32 view: strides s and extents n >= 1 in elements, any sign of stride.  halo_x_stride != 0:
// one more row of that stride on either side (rows -1 and X of an input under PRE_FLAG_HALO_X).  false if an offset leaves
// int64 or the span leaves the address space: such a view addresses nothing a kernel may be given.
inline bool span_of(const void *ptr, const int64_t s[4], const int64_t n[4], int64_t halo_x_stride, Span *out)
{
    int64_t lo = 0, hi = 1;                        // elements [lo, hi) around the base
    for (int d = 0; d < 4; ++d) {
        int64_t e;
        if (__builtin_mul_overflow(s[d], n[d] - 1, &e)) return false;
        if (__builtin_add_overflow(e < 0 ? lo : hi, e, e < 0 ? &lo : &hi)) return false;
    }
    int64_t h;
    if (__builtin_sub_overflow((int64_t)0, halo_x_stride, &h)) return false;
    if (h < 0) h = halo_x_stride;
    if (__builtin_sub_overflow(lo, h, &lo) || __builtin_add_overflow(hi, h, &hi)) return false;
    int64_t blo, bhi;                              // blo <= 0 < bhi
    if (__builtin_mul_overflow(lo, (int64_t)4, &blo) || __builtin_mul_overflow(hi, (int64_t)4, &bhi)) return false;
    const uintptr_t base = (uintptr_t)ptr;
    if ((uint64_t)0 - (uint64_t)blo > base || (uint64_t)bhi > UINTPTR_MAX - base) return false;
    out->lo = base - (uintptr_t)((uint64_t)0 - (uint64_t)blo);
    out->hi = base + (uintptr_t)bhi;
    return true;
}

// (views that touch do not overlap: hi is one past the last byte)
inline bool overlaps(const Span &a, const Span &b) { return a.lo < b.hi && b.lo < a.hi; }

// the offsets inside one sample's [X,Y] plane, (X - 1) * sX + Y at the most, are 32-bit in the kernel
inline bool plane_fits_int32(int64_t sX, int64_t X, int64_t Y)
{
    int64_t e;
    if (__builtin_mul_overflow(sX, X - 1, &e)) return false;
    return e > -0x7fffffffLL && e < 0x7fffffffLL - Y;
}

// The marched kernels address a thread's place in one sample's plane as an UNSIGNED 32-bit byte offset into a buffer
// descriptor: `rows` rows of stride sX >= 0 floats (the tile's overhang and the halo rows included), Y columns, and the 8
// floats a quad and an edge scalar reach past their own cell.  True iff (rows * sX + Y + 8) * 4 < 2^32.
inline bool plane_offsets_fit_u32(int64_t sX, int64_t rows, int64_t Y)
{
    int64_t e;
    if (sX < 0 || rows < 0 || Y < 0 || __builtin_mul_overflow(rows, sX, &e) || __builtin_add_overflow(e, Y, &e)) return false;
    return e < (int64_t)(1LL << 30) - 8;
}

// 16-byte loads and stores along the unit-stride axis: base, row stride and (B > 1) batch stride are whole quads
inline bool aligned16(const void *ptr, int64_t sB, int64_t sX, int64_t B)
{
    return ((uintptr_t)ptr & 15u) == 0 && sX % 4 == 0 && (B == 1 || sB % 4 == 0);
}

// ---- boundary conditions on the (x, y) rim ---------------------------------------------------------------------------
// (Utils/boundary_conditions.py: BoundaryManager.pad_signal followed by a 'valid' conv == a 'same' conv whose out-of-domain
// neighbour is a mapped in-domain cell or a constant.)  For each side: idx >= 0 = row / column to read instead of the cell
// just outside (periodic: the opposite edge; neumann/outflow: the edge itself; symmetric: one inside the edge), idx < 0 =
// the constant val (dirichlet).  Radius-1 stars never see corners.
struct BCInfo { int xlo, xhi, ylo, yhi; float vxlo, vxhi, vylo, vyhi; };

// pre_bc_t side -> (index to read, constant); n = extent of the axis
inline bool bc_side(int mode, float value, int64_t n, bool hi, int *idx, float *val)
{
    *val = 0.f;
    switch (mode) {
    case PRE_BC_CONSTANT: *idx = -1; *val = value; return true;
    case PRE_BC_REPLICATE: *idx = hi ? (int)n - 1 : 0; return true;
    case PRE_BC_PERIODIC: *idx = hi ? 0 : (int)n - 1; return true;
    case PRE_BC_REFLECT: if (n < 2) return false; *idx = hi ? (int)n - 2 : 1; return true;
    default: return false;
    }
}

// top / bottom act on the first spatial axis (X, rows), left / right on the second (Y, columns)
inline bool bc_info(const pre_bc_t *bc, int64_t X, int64_t Y, BCInfo *o)
{
    return bc_side(bc->mode[2], bc->value[2], X, false, &o->xlo, &o->vxlo) && bc_side(bc->mode[3], bc->value[3], X, true, &o->xhi, &o->vxhi) &&
           bc_side(bc->mode[0], bc->value[0], Y, false, &o->ylo, &o->vylo) && bc_side(bc->mode[1], bc->value[1], Y, true, &o->yhi, &o->vyhi);
}

// ---- a dense 3x3 kernel, axes (X, Y), as the cross it must be --------------------------------------------------------
struct Cross { float c, xm, xp, ym, yp; };         // centre, row -1, row +1, column -1, column +1

inline bool cross_from_dense9(const float *K, Cross *k)
{
    if (K[0] != 0.f || K[2] != 0.f || K[6] != 0.f || K[8] != 0.f) return false;
    *k = Cross{K[4], K[1], K[7], K[3], K[5]};
    return true;
}

// ---- the flat form's chunk rule (star_march.h: flat_march_kernel; screen_flat.hip, vjp_flat.hip) ----------------------
constexpr int FLAT_NT = 512, FLAT_H = 32;
#ifndef FLAT_NT_GAIN
#define FLAT_NT_GAIN 8          // a narrower chunk must save this many per cent of a row's lanes to be taken (measured:
                                // profiles/r06/flat_ab_chunk_width.txt - 4 chunks of 320 lost 7 % to 3 of 448 at Nt = 20, 256 wide)
#endif
#ifndef FLAT_NOLDS_NT
#define FLAT_NOLDS_NT 512       // widest chunk of a functor that stages nothing (no LDS, no barrier: the workgroup size is free)
#endif
#ifndef FLAT_HALO_FULL
#define FLAT_HALO_FULL 0        // experiment: 1 = FLAT_H halo quads per side whatever Ty (rounds 2-5)
#endif

// Threads (= quads) per chunk of a merged row of `quads` quads: 512, or 448 / 384 / 320 / 256 when that leaves fewer idle
// lanes in the row's last chunk (the surrogate's Nt = 10 on a 256-wide grid is a row of 640 quads: two chunks of 320
// instead of 512 + 128).  Cost of a row = chunks x (quads + the halo quads staged per chunk: ceil(Ty / 4) per side for a
// functor that stages any field, none otherwise); ties go to the wider chunk.
inline int flat_chunk(long long quads, int Ty, bool staged)
{
    const int halo = FLAT_HALO_FULL ? 2 * FLAT_H : staged ? 2 * ((Ty + 3) / 4 < FLAT_H ? (Ty + 3) / 4 : FLAT_H) : 0;
    int nt = staged ? FLAT_NT : FLAT_NOLDS_NT;
    for (int c = nt - 64; c >= 256; c -= 64)
        if ((quads + c - 1) / c * (c + halo) * 100 < (quads + nt - 1) / nt * (nt + halo) * (100 - FLAT_NT_GAIN)) nt = c;
    return nt;
}

// ---- what every screen of [B,T,X,Y] fields checks of its pre_screen_t / pre_screenflat_t -----------------------------
// null / empty, level count and crops, the count matrix's leading dimension, 32-bit extents (y_room: what the kernel's
// index arithmetic adds to Y) and 32-bit counts.  The layout checks, which differ, stay with the caller.
template <class S>
int screen_args(const pre_field_t *const *fs, int nf, const S *s, int max_levels, int64_t B, int64_t T, int64_t X, int64_t Y,
                int y_room)
{
    if (!s || !s->q || !s->score || !s->count || B <= 0 || T <= 0 || X <= 0 || Y <= 0) return PRE_E_NULL;
    for (int i = 0; i < nf; ++i)
        if (!fs[i] || !fs[i]->ptr) return PRE_E_NULL;
    if (s->nk < 1 || s->nk > max_levels || s->ct < 0 || s->cx < 0 || s->cy < 0) return PRE_E_RANGE;
    if (s->count_ld < B) return PRE_E_NULL;
    if (B > 0x7fffffff || T > 0x7fffffff || X > 0x7fffffff || Y > 0x7fffffff - y_room) return PRE_E_SHAPE;
    if ((double)T * (double)X * (double)Y >= 4294967296.0) return PRE_E_SHAPE;           // the counts are 32-bit
    return PRE_OK;
}

}  // namespace
