// cns_common.h - what the compressible-NS right-hand side (cns_rhs.hip, libcp_pre_cns.so) and its vector-Jacobian product
// (cns_vjp.hip, libcp_pre_cnsvjp.so) share: the tile both kernels own, and the host-side checks of an entry point, written
// once over the planes a pass reads, the planes it writes and the planes its epilogue adds.  The kernels and their staging
// code are their files' own.
#pragma once
#include "common.h"
#include "host_checks.h"
#include "../../include/cp_pre_cns.h"

namespace {

constexpr int NR = PRE_CNS_TILE_ROWS, NC = PRE_CNS_TILE_COLS;
constexpr int QPR = NC / 4;                            // quads in a tile row
constexpr int THREADS = 256;
constexpr int LR = NR + 2;                             // staged rows: -1 .. NR
constexpr int SLOTS = LR * QPR;                        // quads to stage per plane
constexpr int SPT = (SLOTS + THREADS - 1) / THREADS;   // ... per thread
constexpr int C0 = 4;                                  // tile column j sits at C0 + j of a staged row: quads stay 16-byte aligned
constexpr int PITCH = NC + 8;                          // left halo at C0 - 1, right halo at C0 + w (w <= NC columns in the grid)
static_assert(THREADS >= 2 * LR, "the halo cells are staged by the first 2 * LR threads");

// The checks of pre_cns_rhs_f32 / pre_cns_vjp_f32, in the order their headers list the codes, all before any launch.
// rd: nrd <= 2 sets of four planes read (the fields; the cotangents), wr: the four planes written, add: the four planes of
// the epilogue, or null.  On PRE_OK: k[] holds the five crosses of K[], *info the boundary mapping, tilesR x tilesC the
// tiles of a sample and *grid one workgroup per tile of the batch.
inline int cns_check(const pre_cns_plane_t *const *rd, int nrd, const pre_cns_out_t *wr, const pre_cns_plane_t *add,
                     const float *const K[5], Cross *const k[5], const pre_bc_t *bc, BCInfo *info, int64_t B, int64_t X, int64_t Y,
                     int flags, int *tilesR, int *tilesC, unsigned *grid)
{
    if (!wr || !bc) return PRE_E_NULL;
    for (int j = 0; j < nrd; ++j)
        if (!rd[j]) return PRE_E_NULL;
    for (int j = 0; j < 5; ++j)
        if (!K[j]) return PRE_E_NULL;
    // ok(ptr, sB, sX, set, i) of every plane: channel i of set 0 .. nrd - 1 (read), WR (written) or ADD (added, if given)
    enum { WR = 2, ADD = 3, SETS = 4 };
    auto every = [&](auto ok) {
        for (int i = 0; i < 4; ++i) {
            for (int j = 0; j < nrd; ++j)
                if (!ok(rd[j][i].ptr, rd[j][i].sB, rd[j][i].sX, j, i)) return false;
            if (!ok(wr[i].ptr, wr[i].sB, wr[i].sX, WR, i) || (add && !ok(add[i].ptr, add[i].sB, add[i].sX, ADD, i))) return false;
        }
        return true;
    };
    if (!every([](const float *p, int64_t, int64_t, int, int) { return p != nullptr; })) return PRE_E_NULL;
    if (B < 1 || X < 1 || Y < 1) return PRE_E_NULL;
    if (flags != 0) return PRE_E_UNSUPPORTED;
    if (Y % 4 != 0 || X < 2 || Y < 4) return PRE_E_UNSUPPORTED;
    if (!every([&](const float *p, int64_t sB, int64_t sX, int, int) { return aligned16(p, sB, sX, B); })) return PRE_E_UNSUPPORTED;
    for (int j = 0; j < 5; ++j)
        if (!cross_from_dense9(K[j], k[j])) return PRE_E_UNSUPPORTED;
    if (!bc_info(bc, X, Y, info)) return PRE_E_RANGE;

    // int32 cell indices with room for the last tile's overhang, one workgroup per tile in a 1-D grid
    if (B > 0x7fffffff || X > 0x7fffffff - NR || Y > 0x7fffffff - NC) return PRE_E_RANGE;
    const int64_t tR = (X + NR - 1) / NR, tC = (Y + NC - 1) / NC;
    int64_t tiles;
    if (__builtin_mul_overflow(tR, tC, &tiles) || __builtin_mul_overflow(tiles, B, &tiles) || tiles > 0x7fffffff)
        return PRE_E_RANGE;

    Span s[SETS][4];                                                 // by set and channel
    const int64_t n[4] = {B, 1, X, Y};
    if (!every([&](const float *p, int64_t sB, int64_t sX, int set, int i) {
            const int64_t st[4] = {sB, 0, sX, 1};
            return plane_fits_int32(sX, X, Y) && span_of(p, st, n, 0, &s[set][i]);
        }))
        return PRE_E_RANGE;
    // add is either wr itself, channel by channel (a thread reads its cell before it writes it), or somewhere else
    bool in_place = add != nullptr;
    for (int i = 0; add && i < 4; ++i)
        in_place = in_place && add[i].ptr == wr[i].ptr && (B == 1 || add[i].sB == wr[i].sB) && add[i].sX == wr[i].sX;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            for (int set = 0; set < nrd; ++set)                      // a tile's halo (and its fold sources) are other tiles' outputs
                if (overlaps(s[WR][i], s[set][j])) return PRE_E_RANGE;
            if (add && !in_place && overlaps(s[WR][i], s[ADD][j])) return PRE_E_RANGE;
        }
    *tilesR = (int)tR;
    *tilesC = (int)tC;
    *grid = (unsigned)tiles;
    return PRE_OK;
}

}  // namespace
