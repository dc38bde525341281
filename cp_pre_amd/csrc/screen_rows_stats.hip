// screen_rows_stats.hip - per-sample statistics of the 1-D residuals without storing the residual, the second object of
// libcp_pre_screenstats.so (include/cp_pre_screenstats.h; the 2-D residuals are screen_stats.hip's): sum r, sum |r|, sum r^2
// and max |r| over the counted cells of every [Nt,Nx] sample of a [B,Nt,Nx] batch, in either layout.
//
// No kernel of its own: the row march of screen_rows.h on ONE field set, instantiated with the third set policy of
// screen_plane.h (StatSets), with star_march.h's Linear1 and Burgers<MODE> and star_march.o's flags.  The host side is that
// of screen_rows.hip, entry for entry.
#include "screen_rows.h"
#include "../../include/cp_pre_screenstats.h"

namespace {

// prepare_rows' checks in its order, on a joint descriptor of ONE level and no modulation whose level and count pointers
// are placeholders (checked for null only; the geometry is then given no levels: nk = 0, so nothing reads them), then the
// workspace against the query's answer.
int prepare_rows_stats(RGeom &g, StatSets &sets, int *nt_fast, const float *u, const int64_t *strides, const pre_screenstats_t *s,
                       int64_t B, int64_t T, int64_t X, int flags)
{
    if (!s || !s->sums || !s->workspace) return PRE_E_NULL;
    const pre_screen_t j = {reinterpret_cast<const float *>(s->max_abs), 1, nullptr, 0, 0, s->ct, s->cx, s->cy, s->max_abs,
                            s->max_abs, s->sum_ld};
    const int rc = prepare_rows(g, nt_fast, &u, &strides, 1, &j, B, T, X, flags);
    if (rc) return rc;
    if (s->workspace_len < pre_screenstats_workspace_len(PRE_SCREENSTATS_FORM_ROWS, B, T, X, 1)) return PRE_E_NULL;
    g.q = nullptr; g.count = nullptr; g.cld = 0; g.nk = 0; g.mod = nullptr;
    sets.ws = s->workspace; sets.ws_len = s->workspace_len; sets.sums = s->sums; sets.sum_ld = s->sum_ld;
    return PRE_OK;
}

}  // namespace

extern "C" {

int pre_screenstats_rows_stencil2d_f32(const float *u, const int64_t strides[3], const float *tap_w, const int32_t *tap_off,
                                       int ntaps, const pre_screenstats_t *s, int64_t B, int64_t T, int64_t X, int flags,
                                       void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 49) return PRE_E_SHAPE;
    RGeom g;
    StatSets sets;
    int nt_fast = 0;
    int rc = prepare_rows_stats(g, sets, &nt_fast, u, strides, s, B, T, X, flags);
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

int pre_screenstats_rows_burgers_f32(const float *u, const int64_t strides[3], const float *K_t, const float *K_x,
                                     const float *K_xx, float dx, float dt, float nu, float c3, const pre_screenstats_t *s,
                                     int64_t B, int64_t T, int64_t X, int flags, void *stream)
{
    if (!K_t || !K_x || !K_xx) return PRE_E_NULL;
    RGeom g;
    StatSets sets;
    int nt_fast = 0, mode;
    int rc = prepare_rows_stats(g, sets, &nt_fast, u, strides, s, B, T, X, flags);
    if (rc) return rc;
    BurgersParams prm;
    rc = rows_burgers_params(prm, &mode, nt_fast, K_t, K_x, K_xx, dx, dt, nu, c3);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    if (mode == 0) return launch_rows<Burgers<0>>(g, prm, st, sets);
    if (mode == 3) return launch_rows<Burgers<3>>(g, prm, st, sets);
    return launch_rows<Burgers<2>>(g, prm, st, sets);
}

}  // extern "C"
