// screen_cells.hip - the calibrated-set screens of screen_march.hip (Ny-fastest fields) and screen_flat.hip (Nt-fastest
// fields) against PER-CELL sets (libcp_pre_screencells.so, include/cp_pre_screencells.h): per sample, max |r| / m and the
// number of cells with |r| <= q_k[cell] * m[cell] at up to 16 levels, in the launch that evaluates the residual r.  What
// pre_cov_levels_f32 counts with a level field (q_ld != 0), per sample and without a stored residual.
//
// The marches are screen_march.h's and screen_flat.h's, instantiated with their per-cell sets policy (CellSets,
// screen_plane.h), which changes three things in them and nothing else:
//   sets    q is nk level FIELDS.  A thread with a counted cell loads the quads of levels [0, LB) of plane t (load_lev, as
//           load_mod loads the modulation quad: buffer loads, wave-uniform descriptor per level and plane) as the FIRST loads
//           of the plane's step, before the halo of t+1, the own cells of t+2 and the modulation of t+1.  vmcnt retires in
//           issue order, so the wait for the level quads at the end of the plane leaves those later loads in flight, and the
//           quads have the LDS staging, the barrier and the functor to arrive in.  LB = CellsBatch<Fn>: 16 (all of them at
//           once: 64 registers) unless the functor leaves no room; then the quads beyond the first batch are fetched after
//           the functor (load_late), CellsLate<Fn> at a time - here the first batch's size, the default (the specialisations
//           below; DESIGN 4.25 has the measurements; screen_cells_pair.hip sizes the two apart);
//   plane   screen_plane_cells (screen_plane.h): screen_plane with ql[k][j] in place of the wave-uniform qk[k];
//   order   the logical block index is decoded with the sample of a group of CELLS_G fastest, then the tile, the segment,
//           the group.  With the joint screens' order (sample slowest) every sample re-reads nk * 4 bytes of levels per
//           cell from HBM or the Infinity Cache; with a group fastest the workgroups an XCD runs together (xcd_remap makes
//           them contiguous) are CELLS_G samples at ONE tile and read the same level quads from its L2.  Tiles of a sample
//           are CELLS_G apart and still meet in that L2 for their halo rows while CELLS_G is moderate.  The last group is
//           partial when B % CELLS_G != 0: its surplus workgroups return at once.  CELLS_G = 1 is the joint screens' order.
// The host side of an entry is screen_entries.h's: the entry names the views its residual reads and forwards to the body of
// its kind with <Form, Single, CellSets>; the level strides are checked as the modulation's are (prepare_sets), and what is
// not built is in that header's table.
#include "screen_march.h"
#include "screen_flat.h"
#include "../../include/cp_pre_screencells.h"
#include "screen_entries.h"

namespace {

// Level quads held at once, where 16 would not fit the 256 registers of the instantiation without scratch (resources.sh
// screen_cells.hip: every instantiation built has spill 0, scratch 0).  Six-field functors with most fields staged:
template <int M> struct CellsBatch<MHDMomentum<M>, void> { static constexpr int value = PRE_SCREENCELLS_BATCH < 4 ? PRE_SCREENCELLS_BATCH : 4; };
template <int M> struct CellsBatch<MHDEnergy<M>, void> { static constexpr int value = PRE_SCREENCELLS_BATCH < 4 ? PRE_SCREENCELLS_BATCH : 4; };
template <> struct CellsBatch<MHDInduction<2>, void> { static constexpr int value = PRE_SCREENCELLS_BATCH < 8 ? PRE_SCREENCELLS_BATCH : 8; };

}  // namespace

extern "C" {

int pre_screencells_abi_version(void) { return PRE_SCREENCELLS_ABI_VERSION; }
int pre_screencells_sample_group(void) { return CELLS_G; }

// ---------------------------------------------------------------- Ny-fastest fields: screen_march.h
int pre_screencells_stencil3d_f32(const pre_field_t *f, const float *tap_w, const int32_t *tap_off, int ntaps, const pre_screencells_t *s,
                                  int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return stencil3d<NyForm, Single, CellSets>({{f}, 1}, tap_w, tap_off, ntaps, s, B, T, X, Y, flags, stream);
}

int pre_screencells_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                                const pre_screencells_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return linear2<NyForm, Single, CellSets>({{f0, f1}, 2}, K_a, K_b, ratio, s, B, T, X, Y, flags, stream);
}

int pre_screencells_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                    const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                    float dt, float dx, float dy, float nu, const pre_screencells_t *s,
                                    int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return ns_momentum<NyForm, Single, CellSets>({{u, v, p}, 3}, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu, s, B, T, X, Y, flags, stream);
}

int pre_screencells_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y, double gamma,
                            const pre_screencells_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields) return PRE_E_NULL;
    return mhd<NyForm, Single, CellSets>(eq, mhd_views(eq, fields), K_t, K_x, K_y, gamma, s, B, T, X, Y, flags, stream);
}

// ---------------------------------------------------------------- Nt-fastest fields: screen_flat.h
int pre_screencells_flat_stencil3d_f32(const pre_field_t *f, const float *tap_w, const int32_t *tap_off, int ntaps,
                                       const pre_screencellsflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return stencil3d<FlatForm, Single, CellSets>({{f}, 1}, tap_w, tap_off, ntaps, s, B, T, X, Y, flags, stream);
}

int pre_screencells_flat_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                                     const pre_screencellsflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return linear2<FlatForm, Single, CellSets>({{f0, f1}, 2}, K_a, K_b, ratio, s, B, T, X, Y, flags, stream);
}

int pre_screencells_flat_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                         const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                         float dt, float dx, float dy, float nu, const pre_screencellsflat_t *s,
                                         int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return ns_momentum<FlatForm, Single, CellSets>({{u, v, p}, 3}, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu, s, B, T, X, Y, flags, stream);
}

int pre_screencells_flat_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y, double gamma,
                                 const pre_screencellsflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields) return PRE_E_NULL;
    return mhd<FlatForm, Single, CellSets>(eq, mhd_views(eq, fields), K_t, K_x, K_y, gamma, s, B, T, X, Y, flags, stream);
}

}  // extern "C"
