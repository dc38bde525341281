// screen_rows.hip - the calibrated-set screen of the 1-D residuals (libcp_pre_screen1d.so, include/cp_pre_screen1d.h): per
// sample of a [B,Nt,Nx] batch, max |r| / m and the number of cells with |r| <= q_k * m at up to 16 levels, in the launch
// that evaluates the residual r (a ConvOperator of convops_1d, the advection residual, the Burgers residual).
//
// The row march, its split (rows_split), the end of a row and the host checks are screen_rows.h's, shared with
// screen_rows_pair.hip; this unit instantiates them on ONE field set, with star_march.h's Linear1 and Burgers<MODE>.
#include "screen_rows.h"
#include "../../include/cp_pre_screen1d.h"

extern "C" {

int pre_screen1d_abi_version(void) { return PRE_SCREEN1D_ABI_VERSION; }

int pre_screen1d_stencil2d_f32(const float *u, const int64_t strides[3], const float *tap_w, const int32_t *tap_off, int ntaps,
                               const pre_screen_t *s, int64_t B, int64_t T, int64_t X, int flags, void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 49) return PRE_E_SHAPE;
    RGeom g;
    int nt_fast = 0;
    int rc = prepare_rows(g, &nt_fast, &u, &strides, 1, s, B, T, X, flags);
    if (rc) return rc;
    float k9[9];
    bool star;
    rc = rows_dense9_of_taps(tap_w, tap_off, ntaps, k9, &star);
    if (rc) return rc;
    if (!star) return PRE_E_UNSUPPORTED;
    Linear1::Params p;
    rows_star_from_dense9(k9, nt_fast, &p.s);
    return launch_rows<Linear1>(g, p, as_stream(stream));
}

int pre_screen1d_burgers_f32(const float *u, const int64_t strides[3], const float *K_t, const float *K_x, const float *K_xx,
                             float dx, float dt, float nu, float c3, const pre_screen_t *s, int64_t B, int64_t T, int64_t X,
                             int flags, void *stream)
{
    if (!K_t || !K_x || !K_xx) return PRE_E_NULL;
    RGeom g;
    int nt_fast = 0, mode;
    int rc = prepare_rows(g, &nt_fast, &u, &strides, 1, s, B, T, X, flags);
    if (rc) return rc;
    BurgersParams prm;
    rc = rows_burgers_params(prm, &mode, nt_fast, K_t, K_x, K_xx, dx, dt, nu, c3);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    if (mode == 0) return launch_rows<Burgers<0>>(g, prm, st);
    if (mode == 3) return launch_rows<Burgers<3>>(g, prm, st);
    return launch_rows<Burgers<2>>(g, prm, st);
}

}  // extern "C"
