// screen_jorek.hip - the calibrated-set screens of screen_march.hip (Ny-fastest fields) and screen_flat.hip (Nt-fastest
// fields) for the reduced-MHD (JOREK) residuals (libcp_pre_screenjorek.so, include/cp_pre_screenjorek.h): per sample,
// max |r| / m and the number of cells with |r| <= q_k * m at up to 16 levels, in the launch that evaluates r.
//
// Nothing new runs on the device: the marches are screen_march.h's and screen_flat.h's, the functors star_march.h's
// JorekContinuity / JorekTemperature, which take the radius R as one more field of which only the centre value is read (no
// LDS slot, no halo row for it).  The host side is pre_residual_jorek_f32's (star_march.hip) with the set descriptor in place
// of the output: the same kernels, the same four scalars, the same choice of the tap structure - so the residual in registers
// is the one that pass would have stored, given this object's flags are star_march.o's (csrc/Makefile).
//
// Every tap structure of both equations is built in both forms (resources.sh screen_jorek.hip: scratch=0 throughout, DESIGN
// 4.20).  An instantiation with scratch would not be built: its entry would return PRE_E_UNSUPPORTED for that mode.
#include "screen_march.h"
#include "screen_flat.h"
#include "../../include/cp_pre_screenjorek.h"

namespace {

// The kernels, the scalars and the tap structure as pre_residual_jorek_f32 takes them; *mode on the caller's axes.
int jorek_params(JorekParams &prm, int *mode, const float *K_t, const float *K_R, const float *K_Z, const float *K_RR,
                 const float *K_ZZ, const float coef[4])
{
    if (!star_from_dense27(K_t, &prm.Dt) || !star_from_dense27(K_R, &prm.DR) || !star_from_dense27(K_Z, &prm.DZ) ||
        !star_from_dense27(K_RR, &prm.DRR) || !star_from_dense27(K_ZZ, &prm.DZZ))
        return PRE_E_UNSUPPORTED;
    prm.a0 = coef[0]; prm.a1 = coef[1]; prm.a2 = coef[2]; prm.a3 = coef[3];
    // D_RR must fit D_R's compiled tap structure and D_ZZ that of D_Z, else every operator is a general star
    int m = pick_mode(prm.Dt, prm.DR, prm.DZ, nullptr);
    const Shape rr = shape_of(prm.DRR), zz = shape_of(prm.DZZ);
    const bool rr_ok = !rr.t && !rr.y, zz_ok = m == 0 ? (!zz.x && !zz.y) : (!zz.x && !zz.t);
    if (m != 2 && !(rr_ok && zz_ok)) m = 2;
    *mode = m;
    return PRE_OK;
}

}  // namespace

extern "C" {

int pre_screenjorek_abi_version(void) { return PRE_SCREENJOREK_ABI_VERSION; }

int pre_screenjorek_f32(int eq, const pre_field_t fields[3], const pre_field_t *Rb,
                        const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                        const float coef[4], const pre_screen_t *s,
                        int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !Rb || !K_t || !K_R || !K_Z || !K_RR || !K_ZZ || !coef) return PRE_E_NULL;
    if (eq < 0 || eq > 1) return PRE_E_RANGE;
    const pre_field_t *c3[3] = {&fields[0], &fields[1], Rb}, *t4[4] = {&fields[0], &fields[1], &fields[2], Rb};
    SGeom g;
    int rc = eq == 0 ? prepare_screen(g, c3, 3, s, B, T, X, Y, flags) : prepare_screen(g, t4, 4, s, B, T, X, Y, flags);
    if (rc) return rc;
    JorekParams prm;
    int mode;
    rc = jorek_params(prm, &mode, K_t, K_R, K_Z, K_RR, K_ZZ, coef);
    if (rc) return rc;
    Star *stars[5] = {&prm.Dt, &prm.DR, &prm.DZ, &prm.DRR, &prm.DZZ};
    g.tfree = no_t_taps(stars, 5);
    hipStream_t st = as_stream(stream);
    if (eq == 0) return launch_screen_mode<JorekContinuity>(mode, g, prm, st);
    return launch_screen_mode<JorekTemperature>(mode, g, prm, st);
}

int pre_screenjorek_flat_f32(int eq, const pre_field_t fields[3], const pre_field_t *Rb,
                             const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                             const float coef[4], const pre_screenflat_t *s,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !Rb || !K_t || !K_R || !K_Z || !K_RR || !K_ZZ || !coef) return PRE_E_NULL;
    if (eq < 0 || eq > 1) return PRE_E_RANGE;
    const pre_field_t *c3[3] = {&fields[0], &fields[1], Rb}, *t4[4] = {&fields[0], &fields[1], &fields[2], Rb};
    FGeom g;
    int rc = eq == 0 ? prepare_flat(g, c3, 3, s, B, T, X, Y, flags) : prepare_flat(g, t4, 4, s, B, T, X, Y, flags);
    if (rc) return rc;
    JorekParams prm;
    int mode;
    rc = jorek_params(prm, &mode, K_t, K_R, K_Z, K_RR, K_ZZ, coef);      // on the caller's axes
    if (rc) return rc;
    Star *stars[5] = {&prm.Dt, &prm.DR, &prm.DZ, &prm.DRR, &prm.DZZ};
    relabel_stars(stars, 5);
    hipStream_t st = as_stream(stream);
    if (eq == 0) return launch_screen_flat_mode<JorekContinuity>(relabeled_mode(mode, 1), g, prm, st);
    return launch_screen_flat_mode<JorekTemperature>(relabeled_mode(mode, 1), g, prm, st);
}

}  // extern "C"
