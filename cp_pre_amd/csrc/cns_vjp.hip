// libcp_pre_cnsvjp.so (include/cp_pre_cnsvjp.h): the vector-Jacobian product of the compressible-NS right-hand side of
// cns_rhs.hip with respect to (rho, u, v, p), in ONE pass over the four fields and the four cotangent planes, with the
// epilogue gin = add_to + scale * vjp (gfx950 only).  The mathematics and the contract are stated in the header.
//
// The pass takes the forward's shape.  A workgroup of 256 threads owns a tile of NR = 16 rows x NC = 64 columns of one
// sample's plane, one quad of four columns per thread:
//   * it stages the tile of the four fields AND of the four cotangent planes in LDS with a one-cell halo,
//     8 x 18 x 72 floats = 41472 bytes.  A field cell outside the domain is the cell the boundary structure maps it to, or
//     its constant (the pointwise terms need the forward stencils at the centre cells); a cotangent cell outside is not read;
//   * a tile that contains row bc.xlo or bc.xhi also stages row 0 or row X-1 of all eight planes over its columns, a tile
//     that contains column bc.ylo or bc.yhi column 0 or column Y-1 over its rows: the sources of the folds (5120 bytes;
//     other tiles load none of them);
//   * global loads and stores are 16 bytes wide along Ny, and every global load of a thread is issued before its first LDS
//     write: one memory latency per tile;
//   * after ONE barrier each thread walks the cross around each cell of its quad.  A cell n of the cross contributes twice to
//     the gradient at the centre c: through the forward stencils, whose pointwise factors sit at c (s, gm, g0, g3, inv at c
//     times the fields at n: four running sums, no stencil value is ever held), and through the transposes, whose fields
//     w = (a_div, s*u, s*v, -gm*u, -gm*v, gm, g1*inv, g2*inv) are pointwise at n and are formed in registers where they are
//     used.  w of a cell outside the domain is set to zero by a select, not by a product.
// A gather throughout: no atomics, bit-identical reruns.
#include "cns_common.h"
#include "../../include/cp_pre_cnsvjp.h"

namespace {

static_assert(PRE_CNSVJP_TILE_ROWS == NR && PRE_CNSVJP_TILE_COLS == NC, "the forward's tile");
constexpr int NP = 8;                                  // staged planes: rho, u, v, p, g0 .. g3
static_assert(THREADS == NR * QPR, "one thread per quad of the tile");
static_assert(THREADS == 2 * NP * QPR && THREADS == 2 * NP * NR, "one fold quad and one fold cell per thread");

struct Args {
    const float *pl[NP];                               // the fields, then the cotangent planes (batch strides in 64 bits; the
    long long plB[NP];                                 //  offsets inside a sample's plane fit 32 bits: the host checks)
    int plX[NP];
    float *out[4];
    long long outB[4];
    int outX[4];
    const float *add[4];                               // add[0] == nullptr: no epilogue
    long long addB[4];
    int addX[4];
    Cross gx, gy, dx, dy, lap;
    BCInfo bc;
    float gamma, scale;
    int X, Y, tilesR, tilesC;
};

// the weights of the five kernels at one position of the cross
struct Tap { float gx, gy, dx, dy, lap; };

// the four running sums of a cell: d_rho, d_u, d_v, d_p
struct Acc { float rho, u, v, p; };

// the pointwise factors at the centre cell that multiply the forward stencils
struct Coef { float ng0, ngg3, pr, ps, s, gm; };

// the fields under the transposed operators at one cell
struct W { float adiv, su, sv, mu, mv, gm, p1, p2; };

__device__ __forceinline__ W w_of(const float f[NP], float gamma, bool inside)
{
    const float inv = __builtin_amdgcn_rcpf(f[0]);
    const float s = -(f[4] + f[7]), gm = f[5] + f[6];
    W w;
    w.adiv = -f[0] * f[4] - gamma * f[3] * f[7];
    w.su = s * f[1];
    w.sv = s * f[2];
    w.mu = -gm * f[1];
    w.mv = -gm * f[2];
    w.gm = gm;
    w.p1 = f[5] * inv;
    w.p2 = f[6] * inv;
    if (!inside) w = W{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // the mask: rho may be 0 out there, and 0 * inf is NaN
    return w;
}

__device__ __forceinline__ Coef coef_of(const float f[NP], float gamma)
{
    const float inv = __builtin_amdgcn_rcpf(f[0]);
    Coef c;
    c.ng0 = -f[4];
    c.ngg3 = -gamma * f[7];
    c.pr = -inv * inv * f[5];
    c.ps = -inv * inv * f[6];
    c.s = -(f[4] + f[7]);
    c.gm = f[5] + f[6];
    return c;
}

// the forward stencils' share of cell n (fields f, through the boundary mapping) in the gradient at the cell of c;
// t = the FORWARD weights of n's position
__device__ __forceinline__ void forward_share(Acc &a, const Coef &c, const Tap &t, const float f[NP])
{
    const float dv = t.dx * f[1] + t.dy * f[2];
    a.rho += c.ng0 * dv + (c.pr * t.gx + c.ps * t.gy) * f[3];
    a.p += c.ngg3 * dv;
    const float m = c.s * f[0] - c.gm * (f[1] + f[2]);
    a.u += t.gx * m;
    a.v += t.gy * m;
}

// the transposes' share of w at cell n; t = the TRANSPOSED weights of n's position (row +1 carries xm, column +1 ym, ...)
__device__ __forceinline__ void transposed_share(Acc &a, const Tap &t, const W &w)
{
    const float adv = t.gx * w.mu + t.gy * w.mv;
    a.rho += t.gx * w.su + t.gy * w.sv;
    a.u += adv + t.dx * w.adiv + t.lap * w.gm;
    a.v += adv + t.dy * w.adiv;
    a.p += t.gx * w.p1 + t.gy * w.p2;
}

__device__ __forceinline__ float4 axpy(const float4 y, float s, const float4 x)
{
    return make_float4(fmaf(s, x.x, y.x), fmaf(s, x.y, y.y), fmaf(s, x.z, y.z), fmaf(s, x.w, y.w));
}

__global__ void __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) cns_vjp_kernel(const Args a)
{
    __shared__ __attribute__((aligned(16))) float tile[NP][LR * PITCH];
    __shared__ __attribute__((aligned(16))) float foldr[2][NP][NC];   // rows 0 and X-1 over the tile's columns
    __shared__ float foldc[2][NP][NR];                                // columns 0 and Y-1 over the tile's rows

    const int tid = threadIdx.x;
    unsigned bid = blockIdx.x;
    const int tc = (int)(bid % (unsigned)a.tilesC);
    bid /= (unsigned)a.tilesC;
    const int tr = (int)(bid % (unsigned)a.tilesR);
    const long long b = bid / (unsigned)a.tilesR;
    const int r0 = tr * NR, c0 = tc * NC;
    const int h = min(NR, a.X - r0), w = min(NC, a.Y - c0);          // the tile's rows and columns inside the grid; w % 4 == 0

    // ---- every load of the thread, then every LDS write.  Rows -1 .. h of the tile (staged rows 0 .. h + 1), the quads inside the grid
    float4 stage[SPT][NP];
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int s = tid + k * THREADS, lr = s / QPR, lq = s % QPR;
        if (lr > h + 1 || 4 * lq >= w) continue;
        int gx = r0 + lr - 1;
        bool outside = false, constant = false;
        float cv = 0.f;
        if (gx < 0) {
            outside = true;
            constant = a.bc.xlo < 0;
            cv = a.bc.vxlo;
            gx = a.bc.xlo;
        } else if (gx >= a.X) {
            outside = true;
            constant = a.bc.xhi < 0;
            cv = a.bc.vxhi;
            gx = a.bc.xhi;
        }
#pragma unroll
        for (int f = 0; f < NP; ++f) {
            const bool field = f < 4;
            stage[k][f] = field ? make_float4(cv, cv, cv, cv) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (field ? !constant : !outside)
                stage[k][f] = *reinterpret_cast<const float4 *>(a.pl[f] + b * a.plB[f] + (gx * a.plX[f] + c0 + 4 * lq));
        }
    }
    // the cells left and right of those rows: columns c0 - 1 and c0 + w (no quad is staged there)
    const int hlr = tid >> 1, hright = tid & 1;
    const bool hcell = tid < 2 * LR && hlr <= h + 1;
    float halo[NP] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (hcell) {
        int gx = r0 + hlr - 1, gy = hright ? c0 + w : c0 - 1;
        bool outside = false, constant = false;
        float cv = 0.f;
        if (gx < 0) {                                                // (a corner takes the row side's constant first, as the forward)
            outside = true; constant = a.bc.xlo < 0; cv = a.bc.vxlo; gx = a.bc.xlo;
        } else if (gx >= a.X) {
            outside = true; constant = a.bc.xhi < 0; cv = a.bc.vxhi; gx = a.bc.xhi;
        }
        if (!constant) {
            if (gy < 0) {
                outside = true; constant = a.bc.ylo < 0; cv = a.bc.vylo; gy = a.bc.ylo;
            } else if (gy >= a.Y) {
                outside = true; constant = a.bc.yhi < 0; cv = a.bc.vyhi; gy = a.bc.yhi;
            }
        }
#pragma unroll
        for (int f = 0; f < NP; ++f) {
            const bool field = f < 4;
            halo[f] = field ? cv : 0.f;
            if (field ? !constant : !outside) halo[f] = a.pl[f][b * a.plB[f] + (gx * a.plX[f] + gy)];
        }
    }
    // the fold sources: thread = (low / high side, plane, quad of the row or row of the column)
    const int fside = tid / (NP * QPR), fplane = (tid / QPR) % NP, fidx = tid % QPR;
    const int xfold = fside ? a.bc.xhi : a.bc.xlo, yfold = fside ? a.bc.yhi : a.bc.ylo;
    const bool rowfold = xfold >= r0 && xfold < r0 + h && 4 * fidx < w;      // (a constant side has xfold < 0 <= r0)
    const bool colfold = yfold >= c0 && yfold < c0 + w && fidx < h;
    float4 frow = make_float4(0.f, 0.f, 0.f, 0.f);
    float fcol = 0.f;
    if (rowfold || colfold) {
        const float *p = a.pl[fplane] + b * a.plB[fplane];
        const int sX = a.plX[fplane];
        if (rowfold) frow = *reinterpret_cast<const float4 *>(p + ((fside ? a.X - 1 : 0) * sX + c0 + 4 * fidx));
        if (colfold) fcol = p[(r0 + fidx) * sX + (fside ? a.Y - 1 : 0)];
    }

#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int s = tid + k * THREADS, lr = s / QPR, lq = s % QPR;
        if (lr > h + 1 || 4 * lq >= w) continue;
#pragma unroll
        for (int f = 0; f < NP; ++f) *reinterpret_cast<float4 *>(&tile[f][lr * PITCH + C0 + 4 * lq]) = stage[k][f];
    }
    if (hcell) {
#pragma unroll
        for (int f = 0; f < NP; ++f) tile[f][hlr * PITCH + (hright ? C0 + w : C0 - 1)] = halo[f];
    }
    if (rowfold) *reinterpret_cast<float4 *>(&foldr[fside][fplane][4 * fidx]) = frow;
    if (colfold) foldc[fside][fplane][fidx] = fcol;
    __syncthreads();

    const int q = tid % QPR, r = tid / QPR;
    if (4 * q >= w || r >= h) return;
    const int row = r0 + r, col = c0 + 4 * q;
    const int base = (r + 1) * PITCH + C0 + 4 * q;                   // the quad's first cell in a staged plane

    // the centre row: cells col - 1 .. col + 4 of all eight planes
    float mid[6][NP];
#pragma unroll
    for (int f = 0; f < NP; ++f) {
        const float4 m = *reinterpret_cast<const float4 *>(&tile[f][base]);
        mid[0][f] = tile[f][base - 1];
        mid[1][f] = m.x; mid[2][f] = m.y; mid[3][f] = m.z; mid[4][f] = m.w;
        mid[5][f] = tile[f][base + 4];
    }
    Coef cf[4];
    Acc acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cf[j] = coef_of(mid[j + 1], a.gamma);
        acc[j] = Acc{0.f, 0.f, 0.f, 0.f};
    }
    const Tap centre{a.gx.c, a.gy.c, a.dx.c, a.dy.c, a.lap.c};
    const Tap xm{a.gx.xm, a.gy.xm, a.dx.xm, a.dy.xm, a.lap.xm}, xp{a.gx.xp, a.gy.xp, a.dx.xp, a.dy.xp, a.lap.xp};
    const Tap ym{a.gx.ym, a.gy.ym, a.dx.ym, a.dy.ym, a.lap.ym}, yp{a.gx.yp, a.gy.yp, a.dx.yp, a.dy.yp, a.lap.yp};
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        const int gy = col + m - 1;
        const W wm = w_of(mid[m], a.gamma, gy >= 0 && gy < a.Y);
        if (m >= 1 && m <= 4) {                                      // the centre of cell m - 1
            forward_share(acc[m - 1], cf[m - 1], centre, mid[m]);
            transposed_share(acc[m - 1], centre, wm);
        }
        if (m <= 3) {                                                // column -1 of cell m
            forward_share(acc[m], cf[m], ym, mid[m]);
            transposed_share(acc[m], yp, wm);
        }
        if (m >= 2) {                                                // column +1 of cell m - 2
            forward_share(acc[m - 2], cf[m - 2], yp, mid[m]);
            transposed_share(acc[m - 2], ym, wm);
        }
    }
    // the rows above and below (one copy of the code: the loop is not unrolled, the weights are picked on the scalar unit)
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
        float4 n[NP];
#pragma unroll
        for (int f = 0; f < NP; ++f) n[f] = *reinterpret_cast<const float4 *>(&tile[f][base + (side ? PITCH : -PITCH)]);
        const bool inside = side ? row + 1 < a.X : row >= 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float f[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) f[k] = j == 0 ? n[k].x : j == 1 ? n[k].y : j == 2 ? n[k].z : n[k].w;
            forward_share(acc[j], cf[j], side ? xp : xm, f);
            transposed_share(acc[j], side ? xm : xp, w_of(f, a.gamma, inside));
        }
    }
    // the folds: row 0 onto row xlo with the weights of row -1, row X-1 onto row xhi with those of row +1; the columns alike
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
        if (row == (side ? a.bc.xhi : a.bc.xlo)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float f[NP];
#pragma unroll
                for (int k = 0; k < NP; ++k) f[k] = foldr[side][k][4 * q + j];
                transposed_share(acc[j], side ? xp : xm, w_of(f, a.gamma, true));
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (col + j == (side ? a.bc.yhi : a.bc.ylo)) {
                float f[NP];
#pragma unroll
                for (int k = 0; k < NP; ++k) f[k] = foldc[side][k][r];
                transposed_share(acc[j], side ? yp : ym, w_of(f, a.gamma, true));
            }
        }
    }

    const float4 res[4] = {make_float4(acc[0].rho, acc[1].rho, acc[2].rho, acc[3].rho), make_float4(acc[0].u, acc[1].u, acc[2].u, acc[3].u),
                           make_float4(acc[0].v, acc[1].v, acc[2].v, acc[3].v), make_float4(acc[0].p, acc[1].p, acc[2].p, acc[3].p)};
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        float4 v = res[ch];
        if (a.add[0]) v = axpy(*reinterpret_cast<const float4 *>(a.add[ch] + b * a.addB[ch] + (row * a.addX[ch] + col)), a.scale, v);
        *reinterpret_cast<float4 *>(a.out[ch] + b * a.outB[ch] + (row * a.outX[ch] + col)) = v;
    }
}

}  // namespace

extern "C" {

int pre_cnsvjp_abi_version(void) { return PRE_CNSVJP_ABI_VERSION; }

int pre_cns_vjp_f32(const pre_cns_plane_t in[4], const pre_cns_plane_t cot[4], const pre_cns_out_t gin[4], const float *K_gx,
                    const float *K_gy, const float *K_dx, const float *K_dy, const float *K_lap, const pre_bc_t *bc, float gamma,
                    const pre_cns_plane_t *add_to, float scale, int64_t B, int64_t X, int64_t Y, int flags, void *stream)
{
    Args a;
    const pre_cns_plane_t *rd[2] = {in, cot};
    const float *K[5] = {K_gx, K_gy, K_dx, K_dy, K_lap};
    Cross *k[5] = {&a.gx, &a.gy, &a.dx, &a.dy, &a.lap};
    unsigned grid;
    const int rc = cns_check(rd, 2, gin, add_to, K, k, bc, &a.bc, B, X, Y, flags, &a.tilesR, &a.tilesC, &grid);
    if (rc) return rc;

    for (int i = 0; i < 4; ++i) {
        a.pl[i] = in[i].ptr; a.plB[i] = in[i].sB; a.plX[i] = (int)in[i].sX;
        a.pl[4 + i] = cot[i].ptr; a.plB[4 + i] = cot[i].sB; a.plX[4 + i] = (int)cot[i].sX;
        a.out[i] = gin[i].ptr; a.outB[i] = gin[i].sB; a.outX[i] = (int)gin[i].sX;
        a.add[i] = add_to ? add_to[i].ptr : nullptr;
        a.addB[i] = add_to ? add_to[i].sB : 0;
        a.addX[i] = add_to ? (int)add_to[i].sX : 0;
    }
    a.gamma = gamma;
    a.scale = scale;
    a.X = (int)X; a.Y = (int)Y;

    hipLaunchKernelGGL(cns_vjp_kernel, dim3(grid), dim3(THREADS), 0, as_stream(stream), a);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}

}  // extern "C"
