// screen_march.hip - screening predictions against calibrated sets without storing the residual (libcp_pre_screen.so,
// include/cp_pre_screen.h): per sample, max |r| / m and the number of cells with |r| <= q_k * m at up to 16 levels, in the
// launch that evaluates the residual r.
//
// The march templates are star_march.h's (Geom's field layout, Star, Nbr, the functors with their Staged /
// XMASK masks, the lane shifts, the LDS-only barrier, the buffer descriptors, the XCD remap, pick_tseg).  The march (screen_march.h, shared with
// screen_jorek.hip) is march_kernel's: a workgroup of NR x TYQ threads owns NR rows x 4*TYQ columns of ONE sample and marches over a t segment,
// planes t-1, t, t+1 and the in-flight t+2 of its own quads in registers, the current plane staged through LDS for the
// x-neighbours, the y-neighbours from the adjacent lane.  What differs is the end of a plane (screen_plane.h): nothing is stored.  The four
// residual values are masked by the crop (a select), scored against the modulation with the guarded divide of the joint
// score pass (calib.hip: js_update) and counted per level by compare -> wave mask -> population count -> scalar add, as
// coverage_levels.hip counts.  A workgroup works on one sample only, so at the end of its segment its waves are combined
// through LDS and the workgroup issues ONE integer atomicMax on the score's bit pattern and nk integer atomicAdds: both
// are order-independent, so slabs compose and every run gives the same bytes.
//
// The modulation m[T,X,Y] is one more float4 stream, shared by all samples.  Block order: march_kernel's (tiles of a sample
// contiguous per XCD, the sample the slowest index).  The eight XCDs then walk eight different samples through the same
// tile positions at the same pace, so a modulation line that one XCD brings in from HBM is found on die (Infinity Cache)
// by the other seven: at most an eighth of 4 B per cell from HBM even if nothing of it survives until the next sample,
// while the field halos keep meeting in one L2.  (Sample-fastest order would hold a modulation tile in L2 across samples
// but put neighbouring tiles of a sample far apart: every halo row, 2/NR of the input, would be fetched twice.)
//
// The host side of an entry is screen_entries.h's: the entry names the views its residual reads and forwards to the body
// of its kind, here with <NyForm, Single, ScalarSets>.
#include "screen_plane.h"
#include "screen_march.h"      // the kernel, its geometry, launchers and host checks
#include "screen_entries.h"    // the bodies of the entries, shared by the five 2-D screen libraries

extern "C" {

int pre_screen_abi_version(void) { return PRE_SCREEN_ABI_VERSION; }

int pre_screen_stencil3d_f32(const pre_field_t *f, const float *tap_w, const int32_t *tap_off, int ntaps, const pre_screen_t *s,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return stencil3d<NyForm, Single, ScalarSets>({{f}, 1}, tap_w, tap_off, ntaps, s, B, T, X, Y, flags, stream);
}

int pre_screen_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                           const pre_screen_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return linear2<NyForm, Single, ScalarSets>({{f0, f1}, 2}, K_a, K_b, ratio, s, B, T, X, Y, flags, stream);
}

int pre_screen_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                               const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                               float dt, float dx, float dy, float nu, const pre_screen_t *s,
                               int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return ns_momentum<NyForm, Single, ScalarSets>({{u, v, p}, 3}, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu, s, B, T, X, Y, flags,
                                                   stream);
}

int pre_screen_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y, double gamma,
                       const pre_screen_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields) return PRE_E_NULL;
    return mhd<NyForm, Single, ScalarSets>(eq, mhd_views(eq, fields), K_t, K_x, K_y, gamma, s, B, T, X, Y, flags, stream);
}

}  // extern "C"
