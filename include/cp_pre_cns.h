/* cp_pre_cns.h - C ABI of libcp_pre_cns.so: the right-hand side of the reference's compressible Navier-Stokes
 * operator-splitting module (Active_Learning/CNS.py:6-31, class Euler_FV_OS_rhs) in ONE pass over the four fields, with
 * an optional integrator epilogue.
 *
 * vars = (rho, u, v, p), each a plane view [B,X,Y] of one time instance.  With G = (Ggx, Ggy) the gradient's two
 * sub-operators, D = (Ddx, Ddy) the divergence's two and L the Laplacian - five 3x3 kernels applied to the field padded by
 * the boundary condition, as Utils/VectorConvOps_Spatial.py does - the reference computes, in fp32 and in this order,
 *   div   = Ddx(u) + Ddy(v)                       dot(f) = u * Ggx(f) + v * Ggy(f)
 *   mass   = (-rho) * div - dot(rho)
 *   mom_c  = ((-dot(u)) - dot(v) + L(u)) + (1 / rho) * G_c(p)          c = 0, 1
 *   energy = ((-gamma) * p) * div - dot(rho)
 * and returns (mass, mom_0, mom_1, energy).  Nothing of it is "fixed" here: L sees u alone (the reference builds Laplace with
 * scalar=True, v is ignored), both momentum channels carry the same advection and diffusion and differ only in G_c(p) / rho,
 * and the energy line uses the gradient of rho.  Whatever else the reference's constructors do (the spatial 'y' operator
 * differences along Nx, the first-derivative stencil is 1/2-scaled, 'periodic' on all sides maps the high side onto the
 * last cell itself) arrives through the five kernels and the boundary structure the caller hands over: the library takes
 * its taps and its boundary mapping from those, never from a name.
 *
 * Conventions (types and error codes of cp_pre_hip.h):
 *   - the four inputs, the four outputs and the four add_to views are SEPARATE plane views: pointer, batch stride and row
 *     stride in elements, unit stride along Y.  vars[:, 0:4] of a wider tensor, an x- or y-range slice of a larger grid or
 *     four unrelated tensors are read where they lie;
 *   - K_*: dense 3x3 kernels, 9 HOST floats, axes (Nx, Ny).  Each must be a cross (zero corners), else PRE_E_UNSUPPORTED;
 *   - bc: pre_bc_t as for pre_spatial2d_bc_f32: per side an in-domain index to read in place of the cell just outside, or a
 *     constant.  Nothing is padded in memory;
 *   - (1 / rho) is an IEEE fp32 division followed by a multiply, dot a sum of two rounded products;
 *   - epilogue: add_to == NULL: out[c] = rhs[c].  Otherwise out[c] = add_to[c] + step * rhs[c] (one more 4-byte read per
 *     output cell, no extra pass).  out[c] may BE add_to[c] (same pointer and strides);
 *   - what an output cell depends on: the 3x3 box around it in each of the four fields (through the boundary mapping), the
 *     kernels, gamma, and its own add_to cell.  A non-finite input value makes non-finite exactly the cells the reference's
 *     dense F.conv2d makes non-finite: the zero corner taps are multiplied too;
 *   - nothing allocates, nothing synchronises, the one launch is enqueued on `stream`; no state is kept between calls.
 *
 * Returns, all before any launch:
 *   PRE_E_NULL         a null pointer (in, out, a K, bc, any view's ptr) or an extent < 1
 *   PRE_E_UNSUPPORTED  Y % 4 != 0, X < 2, Y < 4, a plane base or a row / batch stride that is not a multiple of 4 floats
 *                      (16 bytes: loads and stores are 16 bytes wide), a kernel off the cross, flags != 0
 *   PRE_E_RANGE        an unknown boundary mode, PRE_BC_REFLECT on an axis of extent < 2, an extent or a tile count beyond
 *                      int32, a view whose offsets inside one sample's plane ((X - 1) * sX + Y) do not fit int32 or whose byte
 *                      offsets overflow int64, an out view whose address range overlaps that of
 *                      an in view (the ranges are compared, not the cells: conservative), an add_to view that overlaps an
 *                      out view without being it
 */
#ifndef CP_PRE_CNS_H
#define CP_PRE_CNS_H

#include <stdint.h>

#include "cp_pre_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tile a workgroup owns (256 threads, one quad of 4 columns each); the tests take their seams from here */
#define PRE_CNS_TILE_ROWS 16
#define PRE_CNS_TILE_COLS 64

typedef struct {
    const float *ptr;
    int64_t sB, sX;            /* element strides of the batch and of the rows; the column stride is 1 */
} pre_cns_plane_t;

typedef struct {
    float *ptr;
    int64_t sB, sX;
} pre_cns_out_t;

#define PRE_CNS_ABI_VERSION 1
int pre_cns_abi_version(void);     /* == PRE_CNS_ABI_VERSION */

int pre_cns_rhs_f32(const pre_cns_plane_t in[4] /*rho,u,v,p*/, const pre_cns_out_t out[4] /*mass,mom_0,mom_1,energy*/,
                    const float *K_gx, const float *K_gy, const float *K_dx, const float *K_dy, const float *K_lap /*host, 9*/,
                    const pre_bc_t *bc /*host*/, float gamma, const pre_cns_plane_t *add_to /*[4] or NULL*/, float step,
                    int64_t B, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_CNS_H */
