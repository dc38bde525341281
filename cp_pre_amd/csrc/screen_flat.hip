// screen_flat.hip - the calibrated-set screen of screen_march.hip for Nt-fastest views of the 2-D residuals
// (libcp_pre_screenflat.so, include/cp_pre_screenflat.h): per sample, max |r| / m and the number of cells with
// |r| <= q_k * m at up to 16 levels, in the launch that evaluates the residual r, for fields whose memory is [B,Nx,Ny,Nt].
//
// The march templates are star_march.h's (Star, Nbr, the functors with their Staged / XMASK masks, the lane
// shifts, the LDS-only barrier, the buffer descriptors, pick_tseg).  The march (screen_flat.h, shared with screen_jorek.hip) is
// flat_march_kernel's up to Fn::eval:
// the kernel axes are relabelled as star_march.h's prepare() relabels them for an Nt-fastest view (marched axis = Nx,
// x = Ny, y = Nt), Ny and Nt are merged into one row of L = Ny*Nt cells, a workgroup owns a chunk of that row of ONE sample
// and marches a segment of Nx with planes t-1, t, t+1 and the in-flight t+2 of its own quads in registers.  x-neighbours
// are Nt cells back / ahead in the merged row, y-neighbours the adjacent cell, masked at row ends.  Only the fields a
// functor reads x-neighbours of go through LDS (halo: ceil(Nt/4) quads per side); the MHD functors stage nothing and run
// without LDS and without a barrier, NS momentum stages u and v.
//
// In place of the store comes screen_march.hip's end of a plane (screen_plane.h): the crop is a select, the score uses the guarded divide of the joint score pass, hw = q_k * m is one
// fp32 multiply with contraction off by pragma (the rest of this file keeps star_march.o's flags, so that the functors
// round as the residual pass does), the counts go compare -> wave mask -> population count -> scalar add.  Marched planes
// outside the crop are not evaluated.  Counted-ness is per LOGICAL cell: a merged-row position m is (y, t) = (m / Nt,
// m % Nt), recovered per cell - a quad straddles a row end when Nt % 4 != 0, so the mask is per element.  At the end of its
// segment the workgroup combines its waves through LDS and issues ONE integer atomicMax on the score's bit pattern and nk
// integer atomicAdds: order-independent, so batch slabs and repeated calls compose and every run gives the same bytes.
//
// The modulation m[T,X,Y] with memory [X,Y,T] is one more float4 stream in the same merged order, loaded only by lanes
// with a counted cell and only for counted planes.
//
// The split (tests/screenflat_helpers.py states it again and names the test seams from it):
//   chunk   flat_chunk(): 512 quads of the merged row per workgroup, or 448 ... 256 when that saves FLAT_NT_GAIN per cent
//           of chunks x (chunk + staged halo quads); the staged halo is 2 * min(32, ceil(Nt/4)) quads for a functor that
//           stages a field, none otherwise (launch_flat's rule);
//   march   pick_tseg(B * chunks, Nx, resident workgroups): the marched axis in segments of tSeg planes.
#include "screen_plane.h"
#include "../../include/cp_pre_screenflat.h"
#include "screen_flat.h"       // the kernel, its geometry, launchers, host checks and the relabelling of the stars

extern "C" {

int pre_screenflat_abi_version(void) { return PRE_SCREENFLAT_ABI_VERSION; }

int pre_screenflat_stencil3d_f32(const pre_field_t *f, const float *tap_w, const int32_t *tap_off, int ntaps,
                                 const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    const pre_field_t *fs[1] = {f};
    FGeom g;
    int rc = prepare_flat(g, fs, 1, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear1::Params p;
    if (!star_of_taps(tap_w, tap_off, ntaps, &p.s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    Star *stars[1] = {&p.s};
    relabel_stars(stars, 1);
    return launch_screen_flat<Linear1>(g, p, as_stream(stream));
}

int pre_screenflat_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                               const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_a || !K_b) return PRE_E_NULL;
    const pre_field_t *fs[2] = {f0, f1};
    FGeom g;
    int rc = prepare_flat(g, fs, 2, s, B, T, X, Y, flags);
    if (rc) return rc;
    Linear2::Params prm;
    if (!star_from_dense27(K_a, &prm.a) || !star_from_dense27(K_b, &prm.b)) return PRE_E_UNSUPPORTED;
    prm.ratio = ratio;
    Star *stars[2] = {&prm.a, &prm.b};
    relabel_stars(stars, 2);
    return launch_screen_flat<Linear2>(g, prm, as_stream(stream));
}

int pre_screenflat_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                   const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                   float dt, float dx, float dy, float nu, const pre_screenflat_t *s,
                                   int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    const pre_field_t *fs[3] = {u, v, p};
    FGeom g;
    int rc = prepare_flat(g, fs, 3, s, B, T, X, Y, flags);
    if (rc) return rc;
    NSParams prm;
    if (!star_from_dense27(K_t, &prm.Dt) || !star_from_dense27(K_x, &prm.Dx) ||
        !star_from_dense27(K_y, &prm.Dy) || !star_from_dense27(K_xx_yy, &prm.L))
        return PRE_E_UNSUPPORTED;
    const int mode = pick_mode(prm.Dt, prm.Dx, prm.Dy, &prm.L);      // on the caller's axes
    prm.dxdy = dx * dy; prm.dtdy = dt * dy; prm.dtdx = dt * dx; prm.nudt = nu * dt;      // (as pre_residual_ns_momentum_f32)
    Star *stars[4] = {&prm.Dt, &prm.Dx, &prm.Dy, &prm.L};
    relabel_stars(stars, 4);
    return launch_screen_flat_mode<NSMomentum>(relabeled_mode(mode, 1), g, prm, as_stream(stream));
}

int pre_screenflat_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y, double gamma,
                           const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields || !K_t || !K_x || !K_y) return PRE_E_NULL;
    if (eq < 0 || eq > 3) return PRE_E_RANGE;
    const pre_field_t *all[6] = {&fields[0], &fields[1], &fields[2], &fields[3], &fields[4], &fields[5]};
    const pre_field_t *c3[3] = {all[0], all[1], all[2]}, *i4[4] = {all[1], all[2], all[4], all[5]};
    FGeom g;
    int rc = eq == 0 ? prepare_flat(g, c3, 3, s, B, T, X, Y, flags)
           : eq == 3 ? prepare_flat(g, i4, 4, s, B, T, X, Y, flags) : prepare_flat(g, all, 6, s, B, T, X, Y, flags);
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
    if (eq == 0) return launch_screen_flat_mode<MHDContinuity>(mode, g, prm, st);
    if (eq == 1) {
        // the general-star instantiation of the momentum functor (six fields, all but rho staged) does not fit 256 registers
        // with the epilogue (20 bytes of scratch): not built, as MHDEnergy<2> in libcp_pre_screen.so; the caller takes its
        // three-pass route
        if (mode == 2) return PRE_E_UNSUPPORTED;
        return mode == 3 ? launch_screen_flat<MHDMomentum<3>>(g, prm, st) : launch_screen_flat<MHDMomentum<4>>(g, prm, st);
    }
    if (eq == 2) return launch_screen_flat_mode<MHDEnergy>(mode, g, prm, st);
    return launch_screen_flat_mode<MHDInduction>(mode, g, prm, st);
}

}  // extern "C"
