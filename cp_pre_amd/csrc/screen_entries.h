// screen_entries.h - the host side of the 2-D calibrated-set screens, stated once for screen_march.hip, screen_flat.hip,
// screen_pair.hip, screen_cells.hip, screen_cells_pair.hip, screen_jorek.hip and screen_jorek_cells.hip: what an entry does between its arguments and its launch.  An entry
// of those files assembles the views its residual reads and forwards to one of the five bodies below (stencil3d, linear2,
// ns_momentum, mhd, jorek), which is templated on what differs between the libraries:
//   Form   NyForm (Ny-fastest fields, screen_march.h) or FlatForm (Nt-fastest fields, screen_flat.h); screen_bc.hip states a
//          third of its own, NyBCForm (NyForm under boundary conditions on the x-y rim), with its rows of Built;
//   W      the functor wrapper: Single (one field set) or Paired (paired_functor.h: d = r(a) - r(b) of two sets);
//   Sets   the set policy of screen_plane.h: ScalarSets (nk levels) or CellSets (nk level fields);
// the set descriptor's type follows from Form and Sets (prepare_sets).  Every body checks in one order: kernel and tap-list
// nulls (PRE_E_NULL; more than 343 taps PRE_E_SHAPE), eq (PRE_E_RANGE), everything prepare_sets checks, kernels off the star
// (PRE_E_UNSUPPORTED, or star_of_taps' own code), a tap structure that is not built (PRE_E_UNSUPPORTED: the table Built).
// Nothing here runs on the device and nothing here chooses a kernel's template arguments but through that table.
#pragma once
#include <type_traits>
#include "screen_march.h"
#include "screen_flat.h"
#include "paired_functor.h"
#include "../../include/cp_pre_screencells.h"

namespace {

// ---- the prepare step: the checks and the geometry of a form, overloaded on the set descriptor ------------------------
int prepare_sets(SGeom &g, ScalarSets &, const pre_field_t *const *fs, int nf, const pre_screen_t *s, int64_t B, int64_t T,
                 int64_t X, int64_t Y, int flags)
{
    return prepare_screen(g, fs, nf, s, B, T, X, Y, flags);
}

int prepare_sets(FGeom &g, ScalarSets &, const pre_field_t *const *fs, int nf, const pre_screenflat_t *s, int64_t B, int64_t T,
                 int64_t X, int64_t Y, int flags)
{
    return prepare_flat(g, fs, nf, s, B, T, X, Y, flags);
}

// per-cell sets: the joint form's checks, then the level strides, checked as the modulation's are
int prepare_sets(SGeom &g, CellSets &sets, const pre_field_t *const *fs, int nf, const pre_screencells_t *s, int64_t B, int64_t T,
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

int prepare_sets(FGeom &g, CellSets &sets, const pre_field_t *const *fs, int nf, const pre_screencellsflat_t *s, int64_t B,
                 int64_t T, int64_t X, int64_t Y, int flags)
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

// ---- the two forms --------------------------------------------------------------------------------------------------
// Geom: the geometry prepare_sets fills.  M0, M1: the reference's and the y-fixed tap structure on the kernel's axes (the
// general star is 2 in both).  finish: what follows once the stars exist; takes the tap structure on the caller's axes
// (pick_mode) and returns it on the kernel's.  launch: the form's launcher.
struct NyForm {
    using Geom = SGeom;
    static constexpr int M0 = 0, M1 = 1;
    static int finish(SGeom &g, Star *const *stars, int n, int mode)
    {
        g.tfree = no_t_taps(stars, n);
        return mode;
    }
    template <class Fn, class P, class Sets>
    static int launch(SGeom &g, const P &prm, hipStream_t st, const Sets &sets) { return launch_screen<Fn>(g, prm, st, sets); }
};

struct FlatForm {
    using Geom = FGeom;
    static constexpr int M0 = 3, M1 = 4;
    static int finish(FGeom &, Star *const *stars, int n, int mode)
    {
        relabel_stars(stars, n);
        return relabeled_mode(mode, 1);
    }
    template <class Fn, class P, class Sets>
    static int launch(FGeom &g, const P &prm, hipStream_t st, const Sets &sets) { return launch_screen_flat<Fn>(g, prm, st, sets); }
};

template <class Fn> using Single = Fn;

// ---- what is built ----------------------------------------------------------------------------------------------------
// Every (form, set policy, functor<tap structure>) is built but the ones below: an instantiation with scratch is not built,
// its tap structure returns PRE_E_UNSUPPORTED and the caller takes its three-pass route (resources.sh on the seven files:
// scratch 0 throughout).  All of them are general stars (<2>) but the y-fixed paired NS momentum.
template <class Form, class Sets, class Fn> struct Built : std::true_type {};
// Ny-fastest, nk levels: the energy functor does not fit 256 registers with the epilogue (24-28 bytes of scratch)
template <> struct Built<NyForm, ScalarSets, MHDEnergy<2>> : std::false_type {};
// Nt-fastest, nk levels: nor does the momentum functor, six fields, all but rho staged (20 bytes of scratch)
template <> struct Built<FlatForm, ScalarSets, MHDMomentum<2>> : std::false_type {};
// per-cell sets: with level quads the momentum functor does not fit even two quads at a time (Ny-fastest 8-16 bytes of
// scratch, Nt-fastest the 20 bytes it has without them), nor the energy functor (24-28 bytes; Nt-fastest 24 at four quads)
template <class Form> struct Built<Form, CellSets, MHDMomentum<2>> : std::false_type {};
template <class Form> struct Built<Form, CellSets, MHDEnergy<2>> : std::false_type {};
// two field sets: the six-view functors need more than 256 registers, as in libcp_pre_pair.so (pair_march.hip: 12-24 bytes
// per lane spilled)
template <class Form> struct Built<Form, ScalarSets, PairedNS<2>> : std::false_type {};
template <class Form> struct Built<Form, ScalarSets, PairedMHDContinuity<2>> : std::false_type {};
// ... and the y-fixed paired NS momentum stages all six fields in the merged-row march: 8 bytes of scratch on its 512-thread
// chunk.  (On the 512-thread tiles of launch_screen the paired NS momentum takes 250-256 registers and the paired MHD
// continuity 169-199, none with scratch, so the tiles stay launch_screen's.)
template <> struct Built<FlatForm, ScalarSets, PairedNS<4>> : std::false_type {};
// two field sets against per-cell sets (screen_cells_pair.hip): the general stars of the six-view functors stay unbuilt (with
// ONE level quad held across the functor and one per later batch, the least there is: the NS momentum 44-48 bytes of scratch
// Ny-fastest and 8 Nt-fastest, the MHD continuity 60-68 and 40), and so does the y-fixed paired NS momentum in BOTH forms
// (8-16 bytes Ny-fastest, 8 Nt-fastest)
template <class Form> struct Built<Form, CellSets, PairedNS<2>> : std::false_type {};
template <class Form> struct Built<Form, CellSets, PairedMHDContinuity<2>> : std::false_type {};
template <> struct Built<NyForm, CellSets, PairedNS<1>> : std::false_type {};
template <> struct Built<FlatForm, CellSets, PairedNS<4>> : std::false_type {};

// per-sample statistics (screen_stats.hip): no level and no modulation registers, but three fp64 accumulators per thread (six
// registers, where the counts of the level screens sit in scalar ones), and the general stars of the two six-field functors do
// not fit with them in either form: the momentum functor 12 bytes of scratch Ny-fastest (all three tiles) and 24 Nt-fastest,
// the energy functor 44-52 and 88
template <class Form> struct Built<Form, StatSets, MHDMomentum<2>> : std::false_type {};
template <class Form> struct Built<Form, StatSets, MHDEnergy<2>> : std::false_type {};

template <class Form, class Fn, class P, class Sets>
int launch_built(typename Form::Geom &g, const P &prm, hipStream_t st, const Sets &sets)
{
    if constexpr (Built<Form, Sets, Fn>::value) return Form::template launch<Fn>(g, prm, st, sets);
    else return PRE_E_UNSUPPORTED;
}

// mode: Form::finish's
template <class Form, template <class> class W, template <int> class FnT, class P, class Sets>
int launch_built_mode(int mode, typename Form::Geom &g, const P &prm, hipStream_t st, const Sets &sets)
{
    if (mode == Form::M0) return launch_built<Form, W<FnT<Form::M0>>>(g, prm, st, sets);
    if (mode == Form::M1) return launch_built<Form, W<FnT<Form::M1>>>(g, prm, st, sets);
    return launch_built<Form, W<FnT<2>>>(g, prm, st, sets);
}

// ---- the views an entry assembles -------------------------------------------------------------------------------------
struct Views { const pre_field_t *fs[MAXF]; int nf; };

// what an ideal-MHD equation reads of rho, u, v, p, Bx, By: continuity the first three, induction u, v, Bx, By, momentum and
// energy (and an eq out of range, which its body declines) all six
Views mhd_views(int eq, const pre_field_t *f)
{
    if (eq == 0) return {{&f[0], &f[1], &f[2]}, 3};
    if (eq == 3) return {{&f[1], &f[2], &f[4], &f[5]}, 4};
    return {{&f[0], &f[1], &f[2], &f[3], &f[4], &f[5]}, 6};
}

// what a JOREK equation reads (screen_jorek.hip, screen_jorek_cells.hip): continuity rho, Phi and the radius, temperature
// rho, Phi, T and the radius (an eq out of range, which its body declines, as temperature)
Views jorek_views(int eq, const pre_field_t *f, const pre_field_t *Rb)
{
    if (eq == 0) return {{&f[0], &f[1], Rb}, 3};
    return {{&f[0], &f[1], &f[2], Rb}, 4};
}

// two field sets of F views each (screen_pair.hip, screen_cells_pair.hip): views [0, F) the set a, [F, 2F) the set b
template <int F>
Views pair_views(const pre_field_t *a, const pre_field_t *b)
{
    Views v = {{}, 2 * F};
    for (int i = 0; i < F; ++i) {
        v.fs[i] = &a[i];
        v.fs[F + i] = &b[i];
    }
    return v;
}

// ---- the five bodies ----------------------------------------------------------------------------------------------------
template <class Form, template <class> class W, class Sets, class S>
int stencil3d(const Views &v, const float *tap_w, const int32_t *tap_off, int ntaps, const S *s, int64_t B, int64_t T, int64_t X,
              int64_t Y, int flags, void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    typename Form::Geom g;
    Sets sets;
    int rc = prepare_sets(g, sets, v.fs, v.nf, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear1::Params prm;
    if (!star_of_taps(tap_w, tap_off, ntaps, &prm.s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    Star *stars[1] = {&prm.s};
    Form::finish(g, stars, 1, 2);
    return launch_built<Form, W<Linear1>>(g, prm, as_stream(stream), sets);
}

template <class Form, template <class> class W, class Sets, class S>
int linear2(const Views &v, const float *K_a, const float *K_b, float ratio, const S *s, int64_t B, int64_t T, int64_t X,
            int64_t Y, int flags, void *stream)
{
    if (!K_a || !K_b) return PRE_E_NULL;
    typename Form::Geom g;
    Sets sets;
    const int rc = prepare_sets(g, sets, v.fs, v.nf, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear2::Params prm;
    if (!star_from_dense27(K_a, &prm.a) || !star_from_dense27(K_b, &prm.b)) return PRE_E_UNSUPPORTED;
    prm.ratio = ratio;
    Star *stars[2] = {&prm.a, &prm.b};
    Form::finish(g, stars, 2, 2);
    return launch_built<Form, W<Linear2>>(g, prm, as_stream(stream), sets);
}

template <class Form, template <class> class W, class Sets, class S>
int ns_momentum(const Views &v, const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy, float dt, float dx,
                float dy, float nu, const S *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    typename Form::Geom g;
    Sets sets;
    int rc = prepare_sets(g, sets, v.fs, v.nf, s, B, T, X, Y, flags);
    if (rc) return rc;
    NSParams prm;
    int mode;
    rc = ns_params(prm, &mode, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu);
    if (rc) return rc;
    Star *stars[4] = {&prm.Dt, &prm.Dx, &prm.Dy, &prm.L};
    mode = Form::finish(g, stars, 4, mode);
    return launch_built_mode<Form, W, NSMomentum>(mode, g, prm, as_stream(stream), sets);
}

// eq 0-3 on one field set; on two, continuity only (twice its three views are what the march takes)
template <class Form, template <class> class W, class Sets, class S>
int mhd(int eq, const Views &v, const float *K_t, const float *K_x, const float *K_y, double gamma, const S *s, int64_t B,
        int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    constexpr bool SINGLE = W<MHDContinuity<0>>::F == MHDContinuity<0>::F;
    if (!K_t || !K_x || !K_y) return PRE_E_NULL;
    if (eq < 0 || eq > (SINGLE ? 3 : 0)) return PRE_E_RANGE;
    typename Form::Geom g;
    Sets sets;
    int rc = prepare_sets(g, sets, v.fs, v.nf, s, B, T, X, Y, flags);
    if (rc) return rc;
    MHDParams prm;
    int mode;
    rc = mhd_params(prm, &mode, K_t, K_x, K_y, gamma);
    if (rc) return rc;
    Star *stars[3] = {&prm.Dt, &prm.Dx, &prm.Dy};
    mode = Form::finish(g, stars, 3, mode);
    hipStream_t st = as_stream(stream);
    if (eq == 0) return launch_built_mode<Form, W, MHDContinuity>(mode, g, prm, st, sets);
    if constexpr (SINGLE) {
        if (eq == 1) return launch_built_mode<Form, W, MHDMomentum>(mode, g, prm, st, sets);
        if (eq == 2) return launch_built_mode<Form, W, MHDEnergy>(mode, g, prm, st, sets);
        return launch_built_mode<Form, W, MHDInduction>(mode, g, prm, st, sets);
    } else {
        return PRE_E_RANGE;      // (not reached: eq == 0 on two sets)
    }
}

// the kernels, the four scalars and the choice of the tap structure as pre_residual_jorek_f32 takes them (jorek_params)
template <class Form, template <class> class W, class Sets, class S>
int jorek(int eq, const Views &v, const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
          const float coef[4], const S *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_t || !K_R || !K_Z || !K_RR || !K_ZZ || !coef) return PRE_E_NULL;
    if (eq < 0 || eq > 1) return PRE_E_RANGE;
    typename Form::Geom g;
    Sets sets;
    int rc = prepare_sets(g, sets, v.fs, v.nf, s, B, T, X, Y, flags);
    if (rc) return rc;
    JorekParams prm;
    int mode;
    rc = jorek_params(prm, &mode, K_t, K_R, K_Z, K_RR, K_ZZ, coef);
    if (rc) return rc;
    Star *stars[5] = {&prm.Dt, &prm.DR, &prm.DZ, &prm.DRR, &prm.DZZ};
    mode = Form::finish(g, stars, 5, mode);
    hipStream_t st = as_stream(stream);
    if (eq == 0) return launch_built_mode<Form, W, JorekContinuity>(mode, g, prm, st, sets);
    return launch_built_mode<Form, W, JorekTemperature>(mode, g, prm, st, sets);
}

}  // namespace
