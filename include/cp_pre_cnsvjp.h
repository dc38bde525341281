/* cp_pre_cnsvjp.h - C ABI of libcp_pre_cnsvjp.so: the vector-Jacobian product of the compressible Navier-Stokes right-hand
 * side of cp_pre_cns.h (Active_Learning/CNS.py:6-31) with respect to its four fields, in ONE pass, with an optional
 * accumulation epilogue.  libcp_pre_cns.so is the forward and stays as it is; this library is its backward.
 *
 * With A_gx, A_gy the gradient's two sub-operators, A_dx, A_dy the divergence's two and A_L the Laplacian - each "pad by the
 * boundary condition, then 3x3 valid correlation", as in cp_pre_cns.h - and g = (g0, g1, g2, g3) the cotangent of
 * (mass, mom_0, mom_1, energy), per cell
 *   div = A_dx u + A_dy v         gm = g1 + g2         s = -(g0 + g3)
 *   a_div = -rho*g0 - gamma*p*g3  inv = 1/rho
 *   t_adv = A_gx^T(-gm*u) + A_gy^T(-gm*v)
 *   d_rho = -div*g0 + A_gx^T(s*u) + A_gy^T(s*v) - inv*inv*(g1*A_gx p + g2*A_gy p)
 *   d_u   = A_dx^T(a_div) + s*A_gx rho - gm*(A_gx u + A_gx v) + t_adv + A_L^T(gm)
 *   d_v   = A_dy^T(a_div) + s*A_gy rho - gm*(A_gy u + A_gy v) + t_adv
 *   d_p   = -gamma*div*g3 + A_gx^T(g1*inv) + A_gy^T(g2*inv)
 * The forward's quirks carry over because they are the expression's: A_L sees u alone, both momentum channels share their
 * advection, the energy line uses grad(rho).
 *
 * Every field w under a transposed operator is a pointwise product of the four fields and g at ONE cell.  The transpose of
 * a cross k = (c, xm, xp, ym, yp) (centre, row -1, row +1, column -1, column +1) under the boundary mapping is a gather, with
 * w taken as 0 outside the domain:
 *   (A^T w)[i,j] = c*w[i,j] + xm*w[i+1,j] + xp*w[i-1,j] + ym*w[i,j+1] + yp*w[i,j-1]
 *      + (i == bc.xlo ? xm*w[0,j]   : 0)      row -1 of row 0 was read from row xlo
 *      + (i == bc.xhi ? xp*w[X-1,j] : 0)
 *      + (j == bc.ylo ? ym*w[i,0]   : 0)
 *      + (j == bc.yhi ? yp*w[i,Y-1] : 0)
 * where bc.* is the index the forward reads in place of the cell just outside (pre_bc_t: replicate = the edge itself, periodic
 * = the opposite edge, reflect = one cell inside), or "constant", which folds nothing.  The folds add, also where they
 * coincide (X == 2 under reflect: xlo == 1, xhi == 0).  The kernels are crosses: there is no corner fold.
 *
 * Conventions (types and error codes of cp_pre_hip.h, plane views of cp_pre_cns.h):
 *   - in (rho, u, v, p), cot (g0..g3), gin (d_rho, d_u, d_v, d_p) and add_to are SEPARATE plane views [B,X,Y]: pointer, batch
 *     stride and row stride in elements, unit stride along Y;
 *   - K_*: dense 3x3 kernels, 9 HOST floats, axes (Nx, Ny); each must be a cross, else PRE_E_UNSUPPORTED;
 *   - plain fp32 with fused multiply-adds, 1/rho by the hardware reciprocal (1 ulp); no rounding order is promised;
 *   - a gather: no atomics, two runs give the same bits;
 *   - epilogue: add_to == NULL: gin[c] = vjp[c] (scale is not read).  Otherwise gin[c] = add_to[c] + scale * vjp[c].
 *     add_to[c] may BE gin[c] (same pointer and strides: gradient accumulation) and may be cot[c] (the backward of an Euler
 *     step, g + h * J^T g);
 *   - what a gradient cell depends on: the cross (not the box) around it in the four fields and in g, through the
 *     boundary mapping for the fields; g and w outside the domain are zero by an explicit mask, never by a product (a constant
 *     side of value 0 maps rho to 0 there, and 0 * (1/0) would be NaN); on the rows xlo / xhi and the columns ylo / yhi also
 *     the edge cell of its column / row that folds onto it; and its own add_to cell.  A non-finite value in a field or
 *     in g therefore reaches the gradient cells of its cross and of its folds and no others: the zero corner taps are NOT
 *     multiplied here, so the footprint is a subset of the one autograd's dense conv backward leaves;
 *   - nothing allocates, nothing synchronises, the one launch is enqueued on `stream`; no state is kept between calls.
 *
 * Returns, all before any launch:
 *   PRE_E_NULL         a null pointer (in, cot, gin, a K, bc, any view's ptr) or an extent < 1
 *   PRE_E_UNSUPPORTED  Y % 4 != 0, X < 2, Y < 4, a plane base or a row / batch stride that is not a multiple of 4 floats
 *                      (16 bytes: loads and stores are 16 bytes wide), a kernel off the cross, flags != 0
 *   PRE_E_RANGE        an unknown boundary mode, PRE_BC_REFLECT on an axis of extent < 2, an extent or a tile count beyond
 *                      int32, a view whose offsets inside one sample's plane ((X - 1) * sX + Y) do not fit int32 or whose byte
 *                      offsets overflow int64, a gin view whose address range overlaps that of an in or a cot view (the
 *                      ranges are compared, not the cells: conservative), an add_to view that overlaps a gin view without
 *                      being it
 */
#ifndef CP_PRE_CNSVJP_H
#define CP_PRE_CNSVJP_H

#include <stdint.h>

#include "cp_pre_cns.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tile a workgroup owns (256 threads, one quad of 4 columns each); the tests take their seams from here */
#define PRE_CNSVJP_TILE_ROWS 16
#define PRE_CNSVJP_TILE_COLS 64

#define PRE_CNSVJP_ABI_VERSION 1
int pre_cnsvjp_abi_version(void);     /* == PRE_CNSVJP_ABI_VERSION */

int pre_cns_vjp_f32(const pre_cns_plane_t in[4] /*rho,u,v,p*/, const pre_cns_plane_t cot[4] /*g0..g3*/,
                    const pre_cns_out_t gin[4] /*d_rho,d_u,d_v,d_p*/,
                    const float *K_gx, const float *K_gy, const float *K_dx, const float *K_dy, const float *K_lap /*host, 9*/,
                    const pre_bc_t *bc /*host*/, float gamma, const pre_cns_plane_t *add_to /*[4] or NULL*/, float scale,
                    int64_t B, int64_t X, int64_t Y, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CP_PRE_CNSVJP_H */
