// screen_bc.hip - the entry points of libcp_pre_screenbc.so (include/cp_pre_screenbc.h): the calibrated-set screen and the
// per-sample statistics of the 2-D residuals under boundary conditions on the x-y rim, without storing the residual.
//
// No march of its own: the BC = true instantiations of screen_march.h's screen_march_kernel with the set policies ScalarSets
// and StatSets, and the bodies of screen_entries.h with one more form, NyBCForm, whose geometry carries the BCInfo
// (host_checks.h: bc_info) the launch hands to the kernel.  Compiled with star_march.o's flags, so a cell whose star stays
// inside the grid gets the bits the zero-pad screens give it.
//
// Out-of-range planes under BC.  As in residual_bc.hip the fills a plane outside [0, T) receives are the sides' constants,
// not zero, and none of them reaches a counted cell: a step runs for t0 <= t < t1 with t1 <= T, so the centre plane, the only
// one LDS is staged from and the only one whose halo row and edge scalars are read, is never out of range (the halo set that
// load_halo(t + 1) fills for t + 1 == t1 is not used); tm / tp read a thread's OWN cells, which are 0 there for every
// thread that counts - the side's constant stands there only in the ghost row x == X of a partial last tile (`gconst`), which
// is not `inb` and so has keep[] false throughout.  The same holds at the cuts of a segment without t-taps (tfree), where [tlo, thi) = [t0, t1).
#include "screen_plane.h"
#include "screen_march.h"
#include "screen_entries.h"
#include "../../include/cp_pre_screenbc.h"

namespace {

// the geometry of the form: screen_march.h's, and the conditions as the kernel takes them
struct BCGeom : SGeom { BCInfo bc; };

// the descriptors of the two set policies with the conditions beside them
struct BCScreen { const pre_screen_t *s; const pre_bc_t *bc; };
struct BCStats { const pre_screenstats_t *s; const pre_bc_t *bc; };

// rows of the tile launch_screen picks for a width
inline int tile_rows(int64_t Y) { return Y >= 192 ? 8 : Y >= 96 ? 16 : 32; }

// what follows prepare_screen under BC: no x-slab, the conditions, the 32-bit in-plane offsets
int prepare_bc(BCGeom &g, const pre_field_t *const *fs, int nf, const pre_bc_t *bc, int64_t X, int64_t Y, int flags)
{
    if (flags & PRE_FLAG_HALO_X) return PRE_E_UNSUPPORTED;
    if (!bc_info(bc, X, Y, &g.bc)) return PRE_E_RANGE;
    for (int i = 0; i < nf; ++i)
        if (!plane_offsets_fit_u32(fs[i]->sX, X + 2 + tile_rows(Y), Y)) return PRE_E_RANGE;
    return PRE_OK;
}

int prepare_sets(BCGeom &g, ScalarSets &, const pre_field_t *const *fs, int nf, const BCScreen *d, int64_t B, int64_t T, int64_t X,
                 int64_t Y, int flags)
{
    if (!d->bc) return PRE_E_NULL;
    const int rc = prepare_screen(g, fs, nf, d->s, B, T, X, Y, flags);
    if (rc) return rc;
    return prepare_bc(g, fs, nf, d->bc, X, Y, flags);
}

// the statistics descriptor as screen_stats.hip prepares it: the joint form's checks on a joint descriptor of one level
// whose level and count pointers are placeholders, then the workspace against the query's answer
int prepare_sets(BCGeom &g, StatSets &sets, const pre_field_t *const *fs, int nf, const BCStats *d, int64_t B, int64_t T, int64_t X,
                 int64_t Y, int flags)
{
    const pre_screenstats_t *s = d->s;
    if (!d->bc || !s || !s->sums || !s->workspace) return PRE_E_NULL;
    const pre_screen_t j = {reinterpret_cast<const float *>(s->max_abs), 1, nullptr, 0, 0, s->ct, s->cx, s->cy, s->max_abs, s->max_abs,
                            s->sum_ld};
    int rc = prepare_screen(g, fs, nf, &j, B, T, X, Y, flags);
    if (rc) return rc;
    if (s->workspace_len < pre_screenbc_stats_workspace_len(B, T, X, Y)) return PRE_E_NULL;
    rc = prepare_bc(g, fs, nf, d->bc, X, Y, flags);
    if (rc) return rc;
    g.q = nullptr; g.count = nullptr; g.cld = 0; g.nk = 0; g.mod = nullptr;
    sets.ws = s->workspace; sets.ws_len = s->workspace_len; sets.sums = s->sums; sets.sum_ld = s->sum_ld;
    return PRE_OK;
}

// NyForm with the BC instantiation of the march
struct NyBCForm {
    using Geom = BCGeom;
    static constexpr int M0 = 0, M1 = 1;
    static int finish(BCGeom &g, Star *const *stars, int n, int mode)
    {
        g.tfree = no_t_taps(stars, n);
        return mode;
    }
    template <class Fn, class P, class Sets>
    static int launch(BCGeom &g, const P &prm, hipStream_t st, const Sets &sets)
    {
        return launch_screen<Fn, Sets, true>(g, prm, st, sets, &g.bc);
    }
};

// not built under BC (the rule of screen_entries.h: nothing that is built uses scratch).  With a second edge scalar per field
// and halo set the general stars of the six-field functors leave the register file for the levels too: 256 registers and
// 24-28 bytes of scratch (momentum), 96-104 (energy) - profiles/screenbc/resources.txt, its last section: this file compiled
// without the two rows below; for the statistics screen_entries.h's rows already hold for every form.  Everything else is
// built, the y-fixed momentum functor next to the fp64 accumulators included (254 registers, no scratch).
template <> struct Built<NyBCForm, ScalarSets, MHDMomentum<2>> : std::false_type {};
template <> struct Built<NyBCForm, ScalarSets, MHDEnergy<2>> : std::false_type {};

}  // namespace

extern "C" {

int pre_screenbc_abi_version(void) { return PRE_SCREENBC_ABI_VERSION; }

int64_t pre_screenbc_stats_workspace_len(int64_t B, int64_t T, int64_t X, int64_t Y)
{
    if (B <= 0 || T <= 0 || X <= 0 || Y <= 0 || B > 0x7fffffff || T > 0x7fffffff || X > 0x7fffffff || Y > 0x7fffffff) return 0;
    return 3 * B * stats_slots_ny(T, X, Y);
}

int pre_screenbc_stencil3d_f32(const pre_field_t *f, const float *tap_w, const int32_t *tap_off, int ntaps, const pre_screen_t *s,
                               const pre_bc_t *bc, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!bc) return PRE_E_NULL;
    const BCScreen d = {s, bc};
    return stencil3d<NyBCForm, Single, ScalarSets>({{f}, 1}, tap_w, tap_off, ntaps, &d, B, T, X, Y, flags, stream);
}

int pre_screenbc_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                             const pre_screen_t *s, const pre_bc_t *bc, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                             void *stream)
{
    if (!bc) return PRE_E_NULL;
    const BCScreen d = {s, bc};
    return linear2<NyBCForm, Single, ScalarSets>({{f0, f1}, 2}, K_a, K_b, ratio, &d, B, T, X, Y, flags, stream);
}

int pre_screenbc_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                 const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                 float dt, float dx, float dy, float nu, const pre_screen_t *s, const pre_bc_t *bc,
                                 int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!bc) return PRE_E_NULL;
    const BCScreen d = {s, bc};
    return ns_momentum<NyBCForm, Single, ScalarSets>({{u, v, p}, 3}, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu, &d, B, T, X, Y, flags,
                                                     stream);
}

int pre_screenbc_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y, double gamma,
                         const pre_screen_t *s, const pre_bc_t *bc, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                         void *stream)
{
    if (!fields || !bc) return PRE_E_NULL;
    const BCScreen d = {s, bc};
    return mhd<NyBCForm, Single, ScalarSets>(eq, mhd_views(eq, fields), K_t, K_x, K_y, gamma, &d, B, T, X, Y, flags, stream);
}

int pre_screenbc_stats_stencil3d_f32(const pre_field_t *f, const float *tap_w, const int32_t *tap_off, int ntaps,
                                     const pre_screenstats_t *s, const pre_bc_t *bc, int64_t B, int64_t T, int64_t X, int64_t Y,
                                     int flags, void *stream)
{
    if (!bc) return PRE_E_NULL;
    const BCStats d = {s, bc};
    return stencil3d<NyBCForm, Single, StatSets>({{f}, 1}, tap_w, tap_off, ntaps, &d, B, T, X, Y, flags, stream);
}

int pre_screenbc_stats_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                                   const pre_screenstats_t *s, const pre_bc_t *bc, int64_t B, int64_t T, int64_t X, int64_t Y,
                                   int flags, void *stream)
{
    if (!bc) return PRE_E_NULL;
    const BCStats d = {s, bc};
    return linear2<NyBCForm, Single, StatSets>({{f0, f1}, 2}, K_a, K_b, ratio, &d, B, T, X, Y, flags, stream);
}

int pre_screenbc_stats_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                       const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                       float dt, float dx, float dy, float nu, const pre_screenstats_t *s, const pre_bc_t *bc,
                                       int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!bc) return PRE_E_NULL;
    const BCStats d = {s, bc};
    return ns_momentum<NyBCForm, Single, StatSets>({{u, v, p}, 3}, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu, &d, B, T, X, Y, flags,
                                                   stream);
}

int pre_screenbc_stats_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y,
                               double gamma, const pre_screenstats_t *s, const pre_bc_t *bc, int64_t B, int64_t T, int64_t X,
                               int64_t Y, int flags, void *stream)
{
    if (!fields || !bc) return PRE_E_NULL;
    const BCStats d = {s, bc};
    return mhd<NyBCForm, Single, StatSets>(eq, mhd_views(eq, fields), K_t, K_x, K_y, gamma, &d, B, T, X, Y, flags, stream);
}

}  // extern "C"
