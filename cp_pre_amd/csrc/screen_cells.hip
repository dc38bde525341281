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
//           the functor, a batch at a time (the specialisations below; DESIGN 4.25 has the measurements);
//   plane   screen_plane_cells (screen_plane.h): screen_plane with ql[k][j] in place of the wave-uniform qk[k];
//   order   the logical block index is decoded with the sample of a group of CELLS_G fastest, then the tile, the segment,
//           the group.  With the joint screens' order (sample slowest) every sample re-reads nk * 4 bytes of levels per
//           cell from HBM or the Infinity Cache; with a group fastest the workgroups an XCD runs together (xcd_remap makes
//           them contiguous) are CELLS_G samples at ONE tile and read the same level quads from its L2.  Tiles of a sample
//           are CELLS_G apart and still meet in that L2 for their halo rows while CELLS_G is moderate.  The last group is
//           partial when B % CELLS_G != 0: its surplus workgroups return at once.  CELLS_G = 1 is the joint screens' order.
// The host side of an entry is its twin's in screen_march.hip / screen_flat.hip with the level strides checked as the
// modulation's are; an instantiation the twin does not build is not built here either.
#include "screen_march.h"
#include "screen_flat.h"
#include "../../include/cp_pre_screencells.h"

namespace {

// Level quads held at once, where 16 would not fit the 256 registers of the instantiation without scratch (resources.sh
// screen_cells.hip: every instantiation built has spill 0, scratch 0).  Six-field functors with most fields staged:
template <int M> struct CellsBatch<MHDMomentum<M>, void> { static constexpr int value = PRE_SCREENCELLS_BATCH < 4 ? PRE_SCREENCELLS_BATCH : 4; };
template <int M> struct CellsBatch<MHDEnergy<M>, void> { static constexpr int value = PRE_SCREENCELLS_BATCH < 4 ? PRE_SCREENCELLS_BATCH : 4; };
template <> struct CellsBatch<MHDInduction<2>, void> { static constexpr int value = PRE_SCREENCELLS_BATCH < 8 ? PRE_SCREENCELLS_BATCH : 8; };

int prepare_cells(SGeom &g, CellSets &sets, const pre_field_t *const *fs, int nf, const pre_screencells_t *s, int64_t B, int64_t T,
                  int64_t X, int64_t Y, int flags)
{
    if (!s) return PRE_E_NULL;
    const pre_screen_t j = {s->levels, s->nk, s->modulation, s->mT, s->mX, s->ct, s->cx, s->cy, s->score, s->count, s->count_ld};
    const int rc = prepare_screen(g, fs, nf, &j, B, T, X, Y, flags);
    if (rc) return rc;
    if (s->lK < 0 || s->lT < 0 || s->lX < 0) return PRE_E_SHAPE;
    sets.qK = s->lK; sets.qT = s->lT; sets.qX = s->lX;
    return PRE_OK;
}

int prepare_cells_flat(FGeom &g, CellSets &sets, const pre_field_t *const *fs, int nf, const pre_screencellsflat_t *s, int64_t B, int64_t T,
                       int64_t X, int64_t Y, int flags)
{
    if (!s) return PRE_E_NULL;
    const pre_screenflat_t j = {s->levels, s->nk, s->modulation, s->mT, s->mX, s->mY, s->ct, s->cx, s->cy, s->score, s->count,
                                s->count_ld};
    const int rc = prepare_flat(g, fs, nf, &j, B, T, X, Y, flags);
    if (rc) return rc;
    if (s->lT != 1 || s->lY != T) return PRE_E_UNSUPPORTED;      // (the fields' in-plane layout, as the modulation)
    if (s->lK < 0 || s->lX < 0) return PRE_E_SHAPE;
    sets.qK = s->lK; sets.qT = s->lX; sets.qX = 0;
    return PRE_OK;
}

}  // namespace

extern "C" {

int pre_screencells_abi_version(void) { return PRE_SCREENCELLS_ABI_VERSION; }
int pre_screencells_sample_group(void) { return CELLS_G; }

// ---------------------------------------------------------------- Ny-fastest fields: screen_march.h
int pre_screencells_stencil3d_f32(const pre_field_t *f, const float *tap_w, const int32_t *tap_off, int ntaps, const pre_screencells_t *s,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    const pre_field_t *fs[1] = {f};
    SGeom g;
    CellSets sets;
    int rc = prepare_cells(g, sets, fs, 1, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear1::Params p;
    if (!star_of_taps(tap_w, tap_off, ntaps, &p.s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    Star *stars[1] = {&p.s};
    g.tfree = no_t_taps(stars, 1);
    return launch_screen<Linear1>(g, p, as_stream(stream), sets);
}

int pre_screencells_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                           const pre_screencells_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_a || !K_b) return PRE_E_NULL;
    const pre_field_t *fs[2] = {f0, f1};
    SGeom g;
    CellSets sets;
    int rc = prepare_cells(g, sets, fs, 2, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear2::Params prm;
    if (!star_from_dense27(K_a, &prm.a) || !star_from_dense27(K_b, &prm.b)) return PRE_E_UNSUPPORTED;
    prm.ratio = ratio;
    Star *stars[2] = {&prm.a, &prm.b};
    g.tfree = no_t_taps(stars, 2);
    return launch_screen<Linear2>(g, prm, as_stream(stream), sets);
}

int pre_screencells_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                               const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                               float dt, float dx, float dy, float nu, const pre_screencells_t *s,
                               int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    const pre_field_t *fs[3] = {u, v, p};
    SGeom g;
    CellSets sets;
    int rc = prepare_cells(g, sets, fs, 3, s, B, T, X, Y, flags);
    if (rc) return rc;
    NSParams prm;
    if (!star_from_dense27(K_t, &prm.Dt) || !star_from_dense27(K_x, &prm.Dx) ||
        !star_from_dense27(K_y, &prm.Dy) || !star_from_dense27(K_xx_yy, &prm.L))
        return PRE_E_UNSUPPORTED;
    const int mode = pick_mode(prm.Dt, prm.Dx, prm.Dy, &prm.L);
    prm.dxdy = dx * dy; prm.dtdy = dt * dy; prm.dtdx = dt * dx; prm.nudt = nu * dt;      // (as pre_residual_ns_momentum_f32)
    Star *stars[4] = {&prm.Dt, &prm.Dx, &prm.Dy, &prm.L};
    g.tfree = no_t_taps(stars, 4);
    return launch_screen_mode<NSMomentum>(mode, g, prm, as_stream(stream), sets);
}

int pre_screencells_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y, double gamma,
                       const pre_screencells_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !K_t || !K_x || !K_y) return PRE_E_NULL;
    if (eq < 0 || eq > 3) return PRE_E_RANGE;
    const pre_field_t *all[6] = {&fields[0], &fields[1], &fields[2], &fields[3], &fields[4], &fields[5]};
    const pre_field_t *c3[3] = {all[0], all[1], all[2]}, *i4[4] = {all[1], all[2], all[4], all[5]};
    SGeom g;
    CellSets sets;
    int rc = eq == 0 ? prepare_cells(g, sets, c3, 3, s, B, T, X, Y, flags)
           : eq == 3 ? prepare_cells(g, sets, i4, 4, s, B, T, X, Y, flags) : prepare_cells(g, sets, all, 6, s, B, T, X, Y, flags);
    if (rc) return rc;
    MHDParams prm;
    if (!star_from_dense27(K_t, &prm.Dt) || !star_from_dense27(K_x, &prm.Dx) || !star_from_dense27(K_y, &prm.Dy))
        return PRE_E_UNSUPPORTED;
    prm.gamma = (float)gamma;
    prm.gm2 = (float)(gamma - 2.0);   // (as pre_residual_mhd_f32)
    const int mode = pick_mode(prm.Dt, prm.Dx, prm.Dy, nullptr);
    Star *stars[3] = {&prm.Dt, &prm.Dx, &prm.Dy};
    g.tfree = no_t_taps(stars, 3);
    hipStream_t st = as_stream(stream);
    if (eq == 0) return launch_screen_mode<MHDContinuity>(mode, g, prm, st, sets);
    if (eq == 1) {
        // with level quads the general-star instantiation of the momentum functor does not fit 256 registers even two quads
        // at a time (8-16 bytes of scratch): not built; the caller takes its three-pass route
        if (mode == 2) return PRE_E_UNSUPPORTED;
        return mode == 0 ? launch_screen<MHDMomentum<0>>(g, prm, st, sets) : launch_screen<MHDMomentum<1>>(g, prm, st, sets);
    }
    if (eq == 2) {
        // the general-star instantiation of the energy functor does not fit 256 registers with the epilogue (24-28 bytes
        // of scratch): not built; the caller takes its three-pass route
        if (mode == 2) return PRE_E_UNSUPPORTED;
        return mode == 0 ? launch_screen<MHDEnergy<0>>(g, prm, st, sets) : launch_screen<MHDEnergy<1>>(g, prm, st, sets);
    }
    return launch_screen_mode<MHDInduction>(mode, g, prm, st, sets);
}

// ---------------------------------------------------------------- Nt-fastest fields: screen_flat.h
int pre_screencells_flat_stencil3d_f32(const pre_field_t *f, const float *tap_w, const int32_t *tap_off, int ntaps,
                                 const pre_screencellsflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    const pre_field_t *fs[1] = {f};
    FGeom g;
    CellSets sets;
    int rc = prepare_cells_flat(g, sets, fs, 1, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear1::Params p;
    if (!star_of_taps(tap_w, tap_off, ntaps, &p.s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    Star *stars[1] = {&p.s};
    relabel_stars(stars, 1);
    return launch_screen_flat<Linear1>(g, p, as_stream(stream), sets);
}

int pre_screencells_flat_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                               const pre_screencellsflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_a || !K_b) return PRE_E_NULL;
    const pre_field_t *fs[2] = {f0, f1};
    FGeom g;
    CellSets sets;
    int rc = prepare_cells_flat(g, sets, fs, 2, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear2::Params prm;
    if (!star_from_dense27(K_a, &prm.a) || !star_from_dense27(K_b, &prm.b)) return PRE_E_UNSUPPORTED;
    prm.ratio = ratio;
    Star *stars[2] = {&prm.a, &prm.b};
    relabel_stars(stars, 2);
    return launch_screen_flat<Linear2>(g, prm, as_stream(stream), sets);
}

int pre_screencells_flat_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                   const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                   float dt, float dx, float dy, float nu, const pre_screencellsflat_t *s,
                                   int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    const pre_field_t *fs[3] = {u, v, p};
    FGeom g;
    CellSets sets;
    int rc = prepare_cells_flat(g, sets, fs, 3, s, B, T, X, Y, flags);
    if (rc) return rc;
    NSParams prm;
    if (!star_from_dense27(K_t, &prm.Dt) || !star_from_dense27(K_x, &prm.Dx) ||
        !star_from_dense27(K_y, &prm.Dy) || !star_from_dense27(K_xx_yy, &prm.L))
        return PRE_E_UNSUPPORTED;
    const int mode = pick_mode(prm.Dt, prm.Dx, prm.Dy, &prm.L);      // on the caller's axes
    prm.dxdy = dx * dy; prm.dtdy = dt * dy; prm.dtdx = dt * dx; prm.nudt = nu * dt;      // (as pre_residual_ns_momentum_f32)
    Star *stars[4] = {&prm.Dt, &prm.Dx, &prm.Dy, &prm.L};
    relabel_stars(stars, 4);
    return launch_screen_flat_mode<NSMomentum>(relabeled_mode(mode, 1), g, prm, as_stream(stream), sets);
}

int pre_screencells_flat_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y, double gamma,
                           const pre_screencellsflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !K_t || !K_x || !K_y) return PRE_E_NULL;
    if (eq < 0 || eq > 3) return PRE_E_RANGE;
    const pre_field_t *all[6] = {&fields[0], &fields[1], &fields[2], &fields[3], &fields[4], &fields[5]};
    const pre_field_t *c3[3] = {all[0], all[1], all[2]}, *i4[4] = {all[1], all[2], all[4], all[5]};
    FGeom g;
    CellSets sets;
    int rc = eq == 0 ? prepare_cells_flat(g, sets, c3, 3, s, B, T, X, Y, flags)
           : eq == 3 ? prepare_cells_flat(g, sets, i4, 4, s, B, T, X, Y, flags) : prepare_cells_flat(g, sets, all, 6, s, B, T, X, Y, flags);
    if (rc) return rc;
    MHDParams prm;
    if (!star_from_dense27(K_t, &prm.Dt) || !star_from_dense27(K_x, &prm.Dx) || !star_from_dense27(K_y, &prm.Dy))
        return PRE_E_UNSUPPORTED;
    prm.gamma = (float)gamma;
    prm.gm2 = (float)(gamma - 2.0);   // (as pre_residual_mhd_f32)
    const int mode = relabeled_mode(pick_mode(prm.Dt, prm.Dx, prm.Dy, nullptr), 1);
    Star *stars[3] = {&prm.Dt, &prm.Dx, &prm.Dy};
    relabel_stars(stars, 3);
    hipStream_t st = as_stream(stream);
    if (eq == 0) return launch_screen_flat_mode<MHDContinuity>(mode, g, prm, st, sets);
    if (eq == 1) {
        // the general-star instantiation of the momentum functor (six fields, all but rho staged) does not fit 256 registers
        // with the epilogue (20 bytes of scratch): not built, as MHDEnergy<2> in libcp_pre_screen.so; the caller takes its
        // three-pass route
        if (mode == 2) return PRE_E_UNSUPPORTED;
        return mode == 3 ? launch_screen_flat<MHDMomentum<3>>(g, prm, st, sets) : launch_screen_flat<MHDMomentum<4>>(g, prm, st, sets);
    }
    if (eq == 2) {
        // the same of the energy functor with level quads (24 bytes of scratch at four quads): not built
        if (mode == 2) return PRE_E_UNSUPPORTED;
        return mode == 3 ? launch_screen_flat<MHDEnergy<3>>(g, prm, st, sets) : launch_screen_flat<MHDEnergy<4>>(g, prm, st, sets);
    }
    return launch_screen_flat_mode<MHDInduction>(mode, g, prm, st, sets);
}

}  // extern "C"
