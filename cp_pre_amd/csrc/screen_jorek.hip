// screen_jorek.hip - the calibrated-set screens of screen_march.hip (Ny-fastest fields) and screen_flat.hip (Nt-fastest
// fields) for the reduced-MHD (JOREK) residuals (libcp_pre_screenjorek.so, include/cp_pre_screenjorek.h): per sample,
// max |r| / m and the number of cells with |r| <= q_k * m at up to 16 levels, in the launch that evaluates r.
//
// Nothing new runs on the device: the marches are screen_march.h's and screen_flat.h's, the functors star_march.h's
// JorekContinuity / JorekTemperature, which take the radius R as one more field of which only the centre value is read (no
// LDS slot, no halo row for it).  The host side is screen_entries.h's body jorek on its jorek_views, which takes the kernels, the four scalars
// and the choice of the tap structure as pre_residual_jorek_f32 does (star_march.h: jorek_params), with the set descriptor in
// place of the output - so the residual in registers is the one that pass would have stored, given this object's flags are
// star_march.o's (csrc/Makefile).
//
// Every tap structure of both equations is built in both forms (resources.sh screen_jorek.hip: scratch=0 throughout, DESIGN
// 4.20).  An instantiation with scratch would not be built: it would get a line in the table Built of screen_entries.h.
#include "screen_march.h"
#include "screen_flat.h"
#include "../../include/cp_pre_screenjorek.h"
#include "screen_entries.h"

extern "C" {

int pre_screenjorek_abi_version(void) { return PRE_SCREENJOREK_ABI_VERSION; }

int pre_screenjorek_f32(int eq, const pre_field_t fields[3], const pre_field_t *Rb,
                        const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                        const float coef[4], const pre_screen_t *s,
                        int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !Rb) return PRE_E_NULL;
    return jorek<NyForm, Single, ScalarSets>(eq, jorek_views(eq, fields, Rb), K_t, K_R, K_Z, K_RR, K_ZZ, coef, s, B, T, X, Y, flags,
                                             stream);
}

int pre_screenjorek_flat_f32(int eq, const pre_field_t fields[3], const pre_field_t *Rb,
                             const float *K_t, const float *K_R, const float *K_Z, const float *K_RR, const float *K_ZZ,
                             const float coef[4], const pre_screenflat_t *s,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !Rb) return PRE_E_NULL;
    return jorek<FlatForm, Single, ScalarSets>(eq, jorek_views(eq, fields, Rb), K_t, K_R, K_Z, K_RR, K_ZZ, coef, s, B, T, X, Y,
                                               flags, stream);
}

}  // extern "C"
