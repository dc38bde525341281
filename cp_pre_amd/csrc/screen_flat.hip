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
//
// The host side of an entry is screen_entries.h's: the entry names the views its residual reads and forwards to the body
// of its kind, here with <FlatForm, Single, ScalarSets>.
#include "screen_plane.h"
#include "../../include/cp_pre_screenflat.h"
#include "screen_flat.h"       // the kernel, its geometry, launchers, host checks and the relabelling of the stars
#include "screen_entries.h"    // the bodies of the entries, shared by the five 2-D screen libraries

extern "C" {

int pre_screenflat_abi_version(void) { return PRE_SCREENFLAT_ABI_VERSION; }

int pre_screenflat_stencil3d_f32(const pre_field_t *f, const float *tap_w, const int32_t *tap_off, int ntaps,
                                 const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return stencil3d<FlatForm, Single, ScalarSets>({{f}, 1}, tap_w, tap_off, ntaps, s, B, T, X, Y, flags, stream);
}

int pre_screenflat_linear2_f32(const pre_field_t *f0, const pre_field_t *f1, const float *K_a, const float *K_b, float ratio,
                               const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return linear2<FlatForm, Single, ScalarSets>({{f0, f1}, 2}, K_a, K_b, ratio, s, B, T, X, Y, flags, stream);
}

int pre_screenflat_ns_momentum_f32(const pre_field_t *u, const pre_field_t *v, const pre_field_t *p,
                                   const float *K_t, const float *K_x, const float *K_y, const float *K_xx_yy,
                                   float dt, float dx, float dy, float nu, const pre_screenflat_t *s,
                                   int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    return ns_momentum<FlatForm, Single, ScalarSets>({{u, v, p}, 3}, K_t, K_x, K_y, K_xx_yy, dt, dx, dy, nu, s, B, T, X, Y, flags,
                                                     stream);
}

int pre_screenflat_mhd_f32(int eq, const pre_field_t fields[6], const float *K_t, const float *K_x, const float *K_y, double gamma,
                           const pre_screenflat_t *s, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, void *stream)
{
    if (!fields) return PRE_E_NULL;
    return mhd<FlatForm, Single, ScalarSets>(eq, mhd_views(eq, fields), K_t, K_x, K_y, gamma, s, B, T, X, Y, flags, stream);
}

}  // extern "C"
