// screen_stats.hip - per-sample statistics of the 2-D residuals without storing the residual (libcp_pre_screenstats.so,
// include/cp_pre_screenstats.h): sum r, sum |r|, sum r^2 and max |r| over the counted cells of every sample, in the launch
// that evaluates the residual r - what the 'PRE' acquisition of the active-learning loops sorts its candidates by.
//
// No kernel of its own: the two 2-D marches (screen_march.h, screen_flat.h) instantiated with the third set policy of
// screen_plane.h, StatSets - no levels, no modulation, three fp64 accumulators per thread in place of the counts, the
// workgroup's partial sums stored to its slot of a caller's workspace and added per sample by a second, tiny launch
// (stats_finish) - and the bodies of screen_entries.h with <Form, Single, StatSets>.  This unit keeps star_march.o's flags,
// so the functors round as the residual passes do.  Not built (the table Built of screen_entries.h): the general stars of
// the MHD momentum and energy functors, which carry scratch in both forms next to the six registers of the fp64
// accumulators; every instantiation that is built has none (csrc/resources.sh, profiles/screenstats/).
//
// The 1-D family is this library's second object, screen_rows_stats.hip.
#include "screen_plane.h"
#include "screen_march.h"
#include "screen_flat.h"
#include "screen_rows.h"       // (host only: stats_slots_rows for the workspace query)
#include "screen_entries.h"
#include "../../include/cp_pre_screenstats.h"

namespace {

// The prepare step of the statistics descriptor: the joint form's checks in the joint form's order, on a joint descriptor
// of ONE level and no modulation whose level and count pointers are placeholders (checked for null only; the geometry is
// then given no levels: nk = 0, so nothing reads them), then the workspace against the query's answer.
template <class J> J stats_as_joint(const pre_screenstats_t *s);
template <> pre_screen_t stats_as_joint<pre_screen_t>(const pre_screenstats_t *s)
{
    return {reinterpret_cast<const float *>(s->max_abs), 1, nullptr, 0, 0, s->ct, s->cx, s->cy, s->max_abs, s->max_abs, s->sum_ld};
}
template <> pre_screenflat_t stats_as_joint<pre_screenflat_t>(const pre_screenstats_t *s)
{
    return {reinterpret_cast<const float *>(s->max_abs), 1, nullptr, 0, 0, 0, s->ct, s->cx, s->cy, s->max_abs, s->max_abs, s->sum_ld};
}

template <class Geom>
void stats_geom(Geom &g, StatSets &sets, const pre_screenstats_t *s)
{
    g.q = nullptr; g.count = nullptr; g.cld = 0; g.nk = 0; g.mod = nullptr;
    sets.ws = s->workspace; sets.ws_len = s->workspace_len; sets.sums = s->sums; sets.sum_ld = s->sum_ld;
}

int prepare_sets(SGeom &g, StatSets &sets, const pre_field_t *const *fs, int nf, const pre_screenstats_t *s, int64_t B, int64_t T,
                 int64_t X, int64_t Y, int flags)
{
    if (!s || !s->sums || !s->workspace) return PRE_E_NULL;
    const pre_screen_t j = stats_as_joint<pre_screen_t>(s);
    const int rc = prepare_screen(g, fs, nf, &j, B, T, X, Y, flags);
    if (rc) return rc;
    if (s->workspace_len < pre_screenstats_workspace_len(PRE_SCREENSTATS_FORM_NY, B, T, X, Y)) return PRE_E_NULL;
    stats_geom(g, sets, s);
    return PRE_OK;
}

int prepare_sets(FGeom &g, StatSets &sets, const pre_field_t *const *fs, int nf, const pre_screenstats_t *s, int64_t B, int64_t T,
                 int64_t X, int64_t Y, int flags)
{
    if (!s || !s->sums || !s->workspace) return PRE_E_NULL;
    const pre_screenflat_t j = stats_as_joint<pre_screenflat_t>(s);
    const int rc = prepare_flat(g, fs, nf, &j, B, T, X, Y, flags);
    if (rc) return rc;
    if (s->workspace_len < pre_screenstats_workspace_len(PRE_SCREENSTATS_FORM_FLAT, B, T, X, Y)) return PRE_E_NULL;
    stats_geom(g, sets, s);
    return PRE_OK;
}

}  // namespace

extern "C" {

int pre_screenstats_abi_version(void) { return PRE_SCREENSTATS_ABI_VERSION; }

int64_t pre_screenstats_workspace_len(int form, int64_t B, int64_t T, int64_t X, int64_t Y)
{
    if (B <= 0 || T <= 0 || X <= 0 || B > 0x7fffffff || T > 0x7fffffff || X > 0x7fffffff) return 0;
    if (form == PRE_SCREENSTATS_FORM_ROWS) {         // either layout: rows Nt x columns Nx, or the other way round
        const long long a = stats_slots_rows(T, X), b = stats_slots_rows(X, T);
        return 3 * B * (a > b ? a : b);
    }
    if (Y <= 0 || Y > 0x7fffffff) return 0;
    if (form == PRE_SCREENSTATS_FORM_NY) return 3 * B * stats_slots_ny(T, X, Y);
    if (form == PRE_SCREENSTATS_FORM_FLAT) return 3 * B * stats_slots_flat(T, X, Y);
    return 0;
}

int pre_screenstats_stencil3d_f32(const pre_field_t *f, const float *tap_w, const int32_t *tap_off, int ntaps,
                                  const pre_screenstats_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return stencil3d<NyForm, Single, StatSets>({{f}, 1}, tap_w, tap_off, ntaps, s, B, T, X, Y, flags, stream);
}

int pre_screenstats_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                                const pre_screenstats_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return linear2<NyForm, Single, StatSets>({{f0, f1}, 2}, K_a, K_b, ratio, s, B, T, X, Y, flags, stream);
}

int pre_screenstats_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                    const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                    float dt, float dx, float dy, float nu, const pre_screenstats_t *s,
                                    int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return ns_momentum<NyForm, Single, StatSets>({{u, v, p}, 3}, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu, s, B, T, X, Y, flags,
                                                 stream);
}

int pre_screenstats_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y, double gamma,
                            const pre_screenstats_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields) return PRE_E_NULL;
    return mhd<NyForm, Single, StatSets>(eq, mhd_views(eq, fields), K_t, K_x, K_y, gamma, s, B, T, X, Y, flags, stream);
}

int pre_screenstats_flat_stencil3d_f32(const pre_field_t *f, const float *tap_w, const int32_t *tap_off, int ntaps,
                                       const pre_screenstats_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                       void *stream)
{
    return stencil3d<FlatForm, Single, StatSets>({{f}, 1}, tap_w, tap_off, ntaps, s, B, T, X, Y, flags, stream);
}

int pre_screenstats_flat_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                                     const pre_screenstats_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                     void *stream)
{
    return linear2<FlatForm, Single, StatSets>({{f0, f1}, 2}, K_a, K_b, ratio, s, B, T, X, Y, flags, stream);
}

int pre_screenstats_flat_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                         const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                         float dt, float dx, float dy, float nu, const pre_screenstats_t *s,
                                         int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return ns_momentum<FlatForm, Single, StatSets>({{u, v, p}, 3}, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu, s, B, T, X, Y, flags,
                                                   stream);
}

int pre_screenstats_flat_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y,
                                 double gamma, const pre_screenstats_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                                 void *stream)
{
    if (!fields) return PRE_E_NULL;
    return mhd<FlatForm, Single, StatSets>(eq, mhd_views(eq, fields), K_t, K_x, K_y, gamma, s, B, T, X, Y, flags, stream);
}

}  // extern "C"
