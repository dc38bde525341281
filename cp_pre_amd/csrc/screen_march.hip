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
#include "screen_plane.h"
#include "screen_march.h"      // the kernel, its geometry, launchers and host checks

extern "C" {

int pre_screen_abi_version(void) { return PRE_SCREEN_ABI_VERSION; }

int pre_screen_stencil3d_f32(const pre_field_t *f, const float *tap_w, const int32_t *tap_off, int ntaps, const pre_screen_t *s,
                             int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    const pre_field_t *fs[1] = {f};
    SGeom g;
    int rc = prepare_screen(g, fs, 1, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear1::Params p;
    if (!star_of_taps(tap_w, tap_off, ntaps, &p.s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    Star *stars[1] = {&p.s};
    g.tfree = no_t_taps(stars, 1);
    return launch_screen<Linear1>(g, p, as_stream(stream));
}

int pre_screen_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                           const pre_screen_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_a || !K_b) return PRE_E_NULL;
    const pre_field_t *fs[2] = {f0, f1};
    SGeom g;
    int rc = prepare_screen(g, fs, 2, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear2::Params prm;
    if (!star_from_dense27(K_a, &prm.a) || !star_from_dense27(K_b, &prm.b)) return PRE_E_UNSUPPORTED;
    prm.ratio = ratio;
    Star *stars[2] = {&prm.a, &prm.b};
    g.tfree = no_t_taps(stars, 2);
    return launch_screen<Linear2>(g, prm, as_stream(stream));
}

int pre_screen_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                               const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                               float dt, float dx, float dy, float nu, const pre_screen_t *s,
                               int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    const pre_field_t *fs[3] = {u, v, p};
    SGeom g;
    int rc = prepare_screen(g, fs, 3, s, B, T, X, Y, flags);
    if (rc) return rc;
    NSParams prm;
    if (!star_from_dense27(K_t, &prm.Dt) || !star_from_dense27(K_x, &prm.Dx) ||
        !star_from_dense27(K_y, &prm.Dy) || !star_from_dense27(K_xx_yy, &prm.L))
        return PRE_E_UNSUPPORTED;
    const int mode = pick_mode(prm.Dt, prm.Dx, prm.Dy, &prm.L);
    prm.dxdy = dx * dy; prm.dtdy = dt * dy; prm.dtdx = dt * dx; prm.nudt = nu * dt;      // (as pre_residual_ns_momentum_f32)
    Star *stars[4] = {&prm.Dt, &prm.Dx, &prm.Dy, &prm.L};
    g.tfree = no_t_taps(stars, 4);
    return launch_screen_mode<NSMomentum>(mode, g, prm, as_stream(stream));
}

int pre_screen_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y, double gamma,
                       const pre_screen_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !K_t || !K_x || !K_y) return PRE_E_NULL;
    if (eq < 0 || eq > 3) return PRE_E_RANGE;
    const pre_field_t *all[6] = {&fields[0], &fields[1], &fields[2], &fields[3], &fields[4], &fields[5]};
    const pre_field_t *c3[3] = {all[0], all[1], all[2]}, *i4[4] = {all[1], all[2], all[4], all[5]};
    SGeom g;
    int rc = eq == 0 ? prepare_screen(g, c3, 3, s, B, T, X, Y, flags)
           : eq == 3 ? prepare_screen(g, i4, 4, s, B, T, X, Y, flags) : prepare_screen(g, all, 6, s, B, T, X, Y, flags);
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
    if (eq == 0) return launch_screen_mode<MHDContinuity>(mode, g, prm, st);
    if (eq == 1) return launch_screen_mode<MHDMomentum>(mode, g, prm, st);
    if (eq == 2) {
        // the general-star instantiation of the energy functor does not fit 256 registers with the epilogue (24-28 bytes
        // of scratch): not built; the caller takes its three-pass route
        if (mode == 2) return PRE_E_UNSUPPORTED;
        return mode == 0 ? launch_screen<MHDEnergy<0>>(g, prm, st) : launch_screen<MHDEnergy<1>>(g, prm, st);
    }
    return launch_screen_mode<MHDInduction>(mode, g, prm, st);
}

}  // extern "C"
