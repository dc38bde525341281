// screen_rows_cells.hip - the calibrated-set screens of screen_rows.hip (one field set) and screen_rows_pair.hip (the
// data-driven scores of two field sets) against PER-CELL sets (libcp_pre_screen1dcells.so, include/cp_pre_screen1dcells.h):
// per sample of a [B,Nt,Nx] batch, max |r| / m and the number of cells with |r| <= q_k[cell] * m[cell] at up to 16 levels, in
// the launch that evaluates the residual r.  What pre_cov_levels_f32 counts with a level field (q_ld != 0), per sample and
// without a stored residual.
//
// The march is screen_rows.h's, instantiated with its per-cell sets policy (CellSets, screen_plane.h): level quads per row
// ahead of the field loads, the end of a row in two parts, a sample group the fastest block index (that header says what
// changes and why).  This unit holds no kernel of its own.  The host side of an entry is its twin's in screen_rows.hip /
// screen_rows_pair.hip: the checks are prepare_rows' on a pre_screen_t rebuilt from the new descriptor, then the level
// strides are checked as the modulation's are.
//
// The file is compiled twice (Makefile), as screen_rows_pair.hip is.  PRE_SCREEN1DCELLS_PART 1, with star_march.o's flags:
// the one-set entries and the paired tap-list entry, which with a constant level field give the bits of
// pre_screen1d_*_f32 / pre_screen1dpair_stencil2d_f32.  PRE_SCREEN1DCELLS_PART 2, without fma contraction: the paired
// Burgers entry, so that both halves of Paired<Burgers> round alike and minus == vars gives exactly 0.
// hw = level * m is uncontracted in both (screen_plane.h).  Every instantiation holds all 16 level quads at once with spill
// 0 and scratch 0 (resources.sh screen_rows_cells.hip with HIPCC_EXTRA of the part; profiles/screen1dcells/resources.txt):
// no functor needs a smaller CellsBatch.
#ifndef PRE_SCREEN1DCELLS_PART
#error "PRE_SCREEN1DCELLS_PART: 1 or 2 (see the Makefile)"
#endif
#include "screen_rows.h"
#include "paired_functor.h"
#include "../../include/cp_pre_screen1dcells.h"

namespace {

// prepare_rows on the joint descriptor this one stands for (every null / range / shape / layout check stated once), then the
// level strides: unit stride on the fields' axis, no negative stride
int prepare_rows_cells(RGeom &g, CellSets &sets, int *nt_fast, const float *const *u, const int64_t *const *strides, int ns,
                       const pre_screen1dcells_t *s, int64_t B, int64_t T, int64_t X, int flags)
{
    if (!s) return PRE_E_NULL;
    const pre_screen_t j = {s->levels, s->nk, s->modulation, s->mT, s->mX, s->ct, s->cx, 0, s->score, s->count, s->count_ld};
    const int rc = prepare_rows(g, nt_fast, u, strides, ns, &j, B, T, X, flags);
    if (rc) return rc;
    const int64_t unit = *nt_fast ? s->lT : s->lX, row = *nt_fast ? s->lX : s->lT;
    if (unit != 1) return PRE_E_UNSUPPORTED;     // (the fields' in-plane layout, as the modulation)
    if (s->lK < 0 || row < 0) return PRE_E_SHAPE;
    sets.qK = s->lK; sets.qT = row; sets.qX = 0;
    return PRE_OK;
}

}  // namespace

extern "C" {

#if PRE_SCREEN1DCELLS_PART == 1

int pre_screen1dcells_abi_version(void) { return PRE_SCREEN1DCELLS_ABI_VERSION; }
int pre_screen1dcells_sample_group(void) { return ROWS_CELLS_G; }

int pre_screen1dcells_stencil2d_f32(const float *u, const int64_t strides[3], const float *tap_w, const int32_t *tap_off, int ntaps,
                                    const pre_screen1dcells_t *s, int64_t B, int64_t T, int64_t X, int flags, void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 49) return PRE_E_SHAPE;
    RGeom g;
    CellSets sets;
    int nt_fast = 0;
    int rc = prepare_rows_cells(g, sets, &nt_fast, &u, &strides, 1, s, B, T, X, flags);
    if (rc) return rc;
    float k9[9];
    bool star;
    rc = rows_dense9_of_taps(tap_w, tap_off, ntaps, k9, &star);
    if (rc) return rc;
    if (!star) return PRE_E_UNSUPPORTED;
    Linear1::Params p;
    rows_star_from_dense9(k9, nt_fast, &p.s);
    return launch_rows<Linear1>(g, p, as_stream(stream), sets);
}

int pre_screen1dcells_burgers_f32(const float *u, const int64_t strides[3], const float *K_t, const float *K_x, const float *K_xx,
                                  float dx, float dt, float nu, float c3, const pre_screen1dcells_t *s, int64_t B, int64_t T,
                                  int64_t X, int flags, void *stream)
{
    if (!K_t || !K_x || !K_xx) return PRE_E_NULL;
    RGeom g;
    CellSets sets;
    int nt_fast = 0, mode;
    int rc = prepare_rows_cells(g, sets, &nt_fast, &u, &strides, 1, s, B, T, X, flags);
    if (rc) return rc;
    BurgersParams prm;
    rc = rows_burgers_params(prm, &mode, nt_fast, K_t, K_x, K_xx, dx, dt, nu, c3);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    if (mode == 0) return launch_rows<Burgers<0>>(g, prm, st, sets);
    if (mode == 3) return launch_rows<Burgers<3>>(g, prm, st, sets);
    return launch_rows<Burgers<2>>(g, prm, st, sets);
}

int pre_screen1dcells_pair_stencil2d_f32(const float *a, const int64_t strides_a[3], const float *b, const int64_t strides_b[3],
                                         const float *tap_w, const int32_t *tap_off, int ntaps, const pre_screen1dcells_t *s,
                                         int64_t B, int64_t T, int64_t X, int flags, void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 49) return PRE_E_SHAPE;
    const float *u[2] = {a, b};
    const int64_t *st[2] = {strides_a, strides_b};
    RGeom g;
    CellSets sets;
    int nt_fast = 0;
    int rc = prepare_rows_cells(g, sets, &nt_fast, u, st, 2, s, B, T, X, flags);
    if (rc) return rc;
    float k9[9];
    bool star;
    rc = rows_dense9_of_taps(tap_w, tap_off, ntaps, k9, &star);
    if (rc) return rc;
    if (!star) return PRE_E_UNSUPPORTED;
    Linear1::Params p;
    rows_star_from_dense9(k9, nt_fast, &p.s);
    return launch_rows<Paired<Linear1>>(g, p, as_stream(stream), sets);
}

#endif  // PRE_SCREEN1DCELLS_PART == 1
#if PRE_SCREEN1DCELLS_PART == 2

int pre_screen1dcells_pair_burgers_f32(const float *a, const int64_t strides_a[3], const float *b, const int64_t strides_b[3],
                                       const float *K_t, const float *K_x, const float *K_xx, float dx, float dt, float nu,
                                       float c3, const pre_screen1dcells_t *s, int64_t B, int64_t T, int64_t X, int flags,
                                       void *stream)
{
    if (!K_t || !K_x || !K_xx) return PRE_E_NULL;
    const float *u[2] = {a, b};
    const int64_t *st[2] = {strides_a, strides_b};
    RGeom g;
    CellSets sets;
    int nt_fast = 0, mode;
    int rc = prepare_rows_cells(g, sets, &nt_fast, u, st, 2, s, B, T, X, flags);
    if (rc) return rc;
    BurgersParams prm;
    rc = rows_burgers_params(prm, &mode, nt_fast, K_t, K_x, K_xx, dx, dt, nu, c3);
    if (rc) return rc;
    hipStream_t hs = as_stream(stream);
    if (mode == 0) return launch_rows<Paired<Burgers<0>>>(g, prm, hs, sets);
    if (mode == 3) return launch_rows<Paired<Burgers<3>>>(g, prm, hs, sets);
    return launch_rows<Paired<Burgers<2>>>(g, prm, hs, sets);
}

#endif  // PRE_SCREEN1DCELLS_PART == 2

}  // extern "C"
