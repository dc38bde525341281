// libcp_pre_cns.so (include/cp_pre_cns.h): the right-hand side of the reference's compressible Navier-Stokes module
// (Active_Learning/CNS.py:6-31) in ONE pass over (rho, u, v, p), with the integrator epilogue out = add_to + step * rhs
// (gfx950 only).  The expression, its quirks and the contract are stated in the header; this file stands alone (it shares no
// template with star_march.h: there is no time march here and no state across launches).
//
// The pass.  A workgroup of 256 threads owns a tile of NR = 16 rows x NC = 64 columns of one sample's plane:
//   * it stages the tile of all four fields in LDS with one halo row above and below and one halo cell left and right
//     (corners included: see below), 4 x 18 x 72 floats = 20736 bytes: LDS would admit seven workgroups per CU, the 100
//     VGPRs admit four, and the loads of one cover the arithmetic of the others.  A cell outside the domain is the cell the boundary structure maps it
//     to, or its constant, read or formed while staging: nothing is padded in memory;
//   * global loads and stores are 16 bytes wide along Ny (the host side declines what is not 16-byte aligned);
//   * after ONE barrier each thread reads the 3 x 6 neighbourhood of its quad in every field from LDS (one 16-byte and two
//     4-byte reads per row), forms the eleven stencil sums of the expression and all four output channels, adds the
//     epilogue's cell if there is one and stores four quads.  Every input cell is read from HBM once per tile, the halo
//     rows (2 in 18) and halo cells a second time, by the neighbouring tile, mostly out of L2.
// The corner cells of the 3x3 box carry no weight (the host side declines a kernel off the cross).  They are staged and
// multiplied by zero all the same, so that a NaN or an inf reaches exactly the cells it reaches through the reference's dense
// F.conv2d, where 0 * inf is NaN: the non-finite footprint of the fused pass is that of the composed route.
#include "cns_common.h"

namespace {

constexpr int TR = THREADS / QPR;                      // rows the threads cover at once
constexpr int RPT = NR / TR;                           // quads a thread computes, TR rows apart
static_assert(RPT >= 1 && NR == RPT * TR, "one thread per quad");

struct Args {
    const float *in[4];                                // (batch strides in 64 bits, applied to the workgroup's sample on the scalar
    long long inB[4];                                  //  unit; the offsets inside a sample's plane fit 32 bits: the host checks)
    int inX[4];
    float *out[4];
    long long outB[4];
    int outX[4];
    const float *add[4];                               // add[0] == nullptr: no epilogue
    long long addB[4];
    int addX[4];
    Cross gx, gy, dx, dy, lap;
    BCInfo bc;
    float gamma, step;
    int X, Y, tilesR, tilesC;
};

// the cell (gx, gy) of a plane, -1 <= gx <= X, -1 <= gy <= Y, through the boundary mapping.  A corner takes the row side's
// constant first: BoundaryManager.pad_signal pads the rows last, over the whole padded width
__device__ __forceinline__ float bc_cell(const float *p, int sX, int gx, int gy, int X, int Y, const BCInfo &bc)
{
    if (gx < 0) {
        if (bc.xlo < 0) return bc.vxlo;
        gx = bc.xlo;
    } else if (gx >= X) {
        if (bc.xhi < 0) return bc.vxhi;
        gx = bc.xhi;
    }
    if (gy < 0) {
        if (bc.ylo < 0) return bc.vylo;
        gy = bc.ylo;
    } else if (gy >= Y) {
        if (bc.yhi < 0) return bc.vyhi;
        gy = bc.yhi;
    }
    return p[gx * sX + gy];
}

// the thread's 3 x 6 neighbourhood in one staged field: rows r-1 .. r+1, columns 4q-1 .. 4q+4
struct Hood { float v[3][6]; };

__device__ __forceinline__ Hood hood_of(const float *t, int r, int q)
{
    Hood h;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int base = (r + i) * PITCH + C0 + 4 * q;
        const float4 m = *reinterpret_cast<const float4 *>(t + base);
        h.v[i][0] = t[base - 1];
        h.v[i][1] = m.x; h.v[i][2] = m.y; h.v[i][3] = m.z; h.v[i][4] = m.w;
        h.v[i][5] = t[base + 4];
    }
    return h;
}

// the zero-weight corners of cell j (1 .. 4) of the neighbourhood: 0 for finite cells, NaN otherwise
__device__ __forceinline__ float corners(const Hood &h, int j)
{
    return fmaf(0.f, h.v[0][j - 1], fmaf(0.f, h.v[0][j + 1], fmaf(0.f, h.v[2][j - 1], 0.f * h.v[2][j + 1])));
}

__device__ __forceinline__ float star(const Cross &k, const Hood &h, int j, float nf)
{
    float s = k.c * h.v[1][j];
    s = fmaf(k.xm, h.v[0][j], s);
    s = fmaf(k.xp, h.v[2][j], s);
    s = fmaf(k.ym, h.v[1][j - 1], s);
    s = fmaf(k.yp, h.v[1][j + 1], s);
    return s + nf;
}

// The reference's expression in the reference's order, every product and every sum rounded on its own, in the three steps
// the fields arrive in (u and v, then rho, then p), so that only a handful of values per cell outlive a field's neighbourhood
struct Cell { float u, v, div, adv, dot_rho, inv; };

__device__ __forceinline__ float dot2(float u, float gx, float v, float gy)
{
#pragma clang fp contract(off)
    return u * gx + v * gy;
}

__device__ __forceinline__ void after_uv(Cell &c, float gx_u, float gy_u, float dx_u, float lap_u, float gx_v, float gy_v, float dy_v)
{
#pragma clang fp contract(off)
    c.div = dx_u + dy_v;
    c.adv = (-dot2(c.u, gx_u, c.v, gy_u)) - dot2(c.u, gx_v, c.v, gy_v) + lap_u;
}

__device__ __forceinline__ float mass_of(Cell &c, float rho, float gx_rho, float gy_rho)
{
#pragma clang fp contract(off)
    c.dot_rho = dot2(c.u, gx_rho, c.v, gy_rho);
    c.inv = __fdiv_rn(1.f, rho);
    return (-rho) * c.div - c.dot_rho;
}

__device__ __forceinline__ float momentum_of(const Cell &c, float g_p)
{
#pragma clang fp contract(off)
    return c.adv + c.inv * g_p;
}

__device__ __forceinline__ float energy_of(const Cell &c, float gamma, float p)
{
#pragma clang fp contract(off)
    return ((-gamma) * p) * c.div - c.dot_rho;
}

__device__ __forceinline__ float4 axpy(const float4 y, float step, const float4 x)
{
#pragma clang fp contract(off)
    return make_float4(y.x + step * x.x, y.y + step * x.y, y.z + step * x.z, y.w + step * x.w);
}

__global__ void __launch_bounds__(THREADS) cns_rhs_kernel(const Args a)
{
    __shared__ __attribute__((aligned(16))) float tile[4][LR * PITCH];

    const int tid = threadIdx.x;
    unsigned bid = blockIdx.x;
    const int tc = (int)(bid % (unsigned)a.tilesC);
    bid /= (unsigned)a.tilesC;
    const int tr = (int)(bid % (unsigned)a.tilesR);
    const long long b = bid / (unsigned)a.tilesR;
    const int r0 = tr * NR, c0 = tc * NC;
    const int h = min(NR, a.X - r0), w = min(NC, a.Y - c0);          // the tile's rows and columns inside the grid; w % 4 == 0

    // rows -1 .. h of the tile (staged rows 0 .. h + 1), the quads inside the grid.  Every load of the thread, the halo cells' below
    // included, is issued before the first value is written to LDS: one memory latency per tile, not two
    float4 stage[SPT][4];
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int s = tid + k * THREADS, lr = s / QPR, lq = s % QPR;
        if (lr > h + 1 || 4 * lq >= w) continue;
        int gx = r0 + lr - 1;
        bool constant = false;
        float cv = 0.f;
        if (gx < 0) {
            constant = a.bc.xlo < 0;
            cv = a.bc.vxlo;
            gx = a.bc.xlo;
        } else if (gx >= a.X) {
            constant = a.bc.xhi < 0;
            cv = a.bc.vxhi;
            gx = a.bc.xhi;
        }
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            stage[k][f] = make_float4(cv, cv, cv, cv);
            if (!constant) stage[k][f] = *reinterpret_cast<const float4 *>(a.in[f] + b * a.inB[f] + (gx * a.inX[f] + c0 + 4 * lq));
        }
    }
    // the cells left and right of those rows: columns c0 - 1 and c0 + w (no quad is staged there)
    const int hlr = tid >> 1, hright = tid & 1;
    const bool hcell = tid < 2 * LR && hlr <= h + 1;
    float halo[4] = {0.f, 0.f, 0.f, 0.f};
    if (hcell) {
#pragma unroll
        for (int f = 0; f < 4; ++f)
            halo[f] = bc_cell(a.in[f] + b * a.inB[f], a.inX[f], r0 + hlr - 1, hright ? c0 + w : c0 - 1, a.X, a.Y, a.bc);
    }
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int s = tid + k * THREADS, lr = s / QPR, lq = s % QPR;
        if (lr > h + 1 || 4 * lq >= w) continue;
#pragma unroll
        for (int f = 0; f < 4; ++f) *reinterpret_cast<float4 *>(&tile[f][lr * PITCH + C0 + 4 * lq]) = stage[k][f];
    }
    if (hcell) {
#pragma unroll
        for (int f = 0; f < 4; ++f) tile[f][hlr * PITCH + (hright ? C0 + w : C0 - 1)] = halo[f];
    }
    __syncthreads();

    const int q = tid % QPR;
    if (4 * q >= w) return;
#pragma unroll 1
    for (int r = tid / QPR; r < h; r += TR) {
    Cell c[4];
    float4 res[4];                                                   // the four channels of the quad
    {
        float gx_u[4], gy_u[4], dx_u[4], lap_u[4];
        {
            const Hood n = hood_of(tile[1], r, q);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float nf = corners(n, j + 1);
                c[j].u = n.v[1][j + 1];
                gx_u[j] = star(a.gx, n, j + 1, nf);
                gy_u[j] = star(a.gy, n, j + 1, nf);
                dx_u[j] = star(a.dx, n, j + 1, nf);
                lap_u[j] = star(a.lap, n, j + 1, nf);
            }
        }
        const Hood n = hood_of(tile[2], r, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float nf = corners(n, j + 1);
            c[j].v = n.v[1][j + 1];
            after_uv(c[j], gx_u[j], gy_u[j], dx_u[j], lap_u[j], star(a.gx, n, j + 1, nf), star(a.gy, n, j + 1, nf),
                     star(a.dy, n, j + 1, nf));
        }
    }
    {
        const Hood n = hood_of(tile[0], r, q);
        float m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float nf = corners(n, j + 1);
            m[j] = mass_of(c[j], n.v[1][j + 1], star(a.gx, n, j + 1, nf), star(a.gy, n, j + 1, nf));
        }
        res[0] = make_float4(m[0], m[1], m[2], m[3]);
    }
    {
        const Hood n = hood_of(tile[3], r, q);
        float m0[4], m1[4], e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float nf = corners(n, j + 1);
            m0[j] = momentum_of(c[j], star(a.gx, n, j + 1, nf));
            m1[j] = momentum_of(c[j], star(a.gy, n, j + 1, nf));
            e[j] = energy_of(c[j], a.gamma, n.v[1][j + 1]);
        }
        res[1] = make_float4(m0[0], m0[1], m0[2], m0[3]);
        res[2] = make_float4(m1[0], m1[1], m1[2], m1[3]);
        res[3] = make_float4(e[0], e[1], e[2], e[3]);
    }

    const int row = r0 + r;
    const int col = c0 + 4 * q;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        float4 v = res[ch];
        if (a.add[0]) v = axpy(*reinterpret_cast<const float4 *>(a.add[ch] + b * a.addB[ch] + (row * a.addX[ch] + col)), a.step, v);
        *reinterpret_cast<float4 *>(a.out[ch] + b * a.outB[ch] + (row * a.outX[ch] + col)) = v;
    }
    }
}

}  // namespace

extern "C" {

int pre_cns_abi_version(void) { return PRE_CNS_ABI_VERSION; }

int pre_cns_rhs_f32(const pre_cns_plane_t in[4], const pre_cns_out_t out[4], const float *K_gx, const float *K_gy,
                    const float *K_dx, const float *K_dy, const float *K_lap, const pre_bc_t *bc, float gamma,
                    const pre_cns_plane_t *add_to, float step, int64_t B, int64_t X, int64_t Y, int flags, void *stream)
{
    Args a;
    const pre_cns_plane_t *rd[1] = {in};
    const float *K[5] = {K_gx, K_gy, K_dx, K_dy, K_lap};
    Cross *k[5] = {&a.gx, &a.gy, &a.dx, &a.dy, &a.lap};
    unsigned grid;
    const int rc = cns_check(rd, 1, out, add_to, K, k, bc, &a.bc, B, X, Y, flags, &a.tilesR, &a.tilesC, &grid);
    if (rc) return rc;

    for (int i = 0; i < 4; ++i) {
        a.in[i] = in[i].ptr; a.inB[i] = in[i].sB; a.inX[i] = (int)in[i].sX;
        a.out[i] = out[i].ptr; a.outB[i] = out[i].sB; a.outX[i] = (int)out[i].sX;
        a.add[i] = add_to ? add_to[i].ptr : nullptr;
        a.addB[i] = add_to ? add_to[i].sB : 0;
        a.addX[i] = add_to ? (int)add_to[i].sX : 0;
    }
    a.gamma = gamma;
    a.step = step;
    a.X = (int)X; a.Y = (int)Y;

    hipLaunchKernelGGL(cns_rhs_kernel, dim3(grid), dim3(THREADS), 0, as_stream(stream), a);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}

}  // extern "C"
