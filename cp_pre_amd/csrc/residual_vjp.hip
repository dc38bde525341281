// residual_vjp.hip - vector-Jacobian products of the PDE residuals and the deterministic sum of squares of a residual
// (libcp_pre_vjp.so, include/cp_pre_vjp.h): what a physics-informed loss mean(r^2) needs for its backward pass.
//
// The march (vjp_march_kernel, its geometry, launch and host-side checks) is vjp_march.h's, shared with vjp_mhd.hip.
// The functors of the linear operators and of NS momentum, with the folding of their stars, are vjp_functors.h's (shared
// with vjp_flat.hip); the Burgers functor has its only user here.
#include "vjp_march.h"

namespace {

// ------------------------------------------------------------------ the functor of Burgers: n[0] is gg, r[] the gradient
// r = dx*D_t(u) + dt*u*D_x(u) - nu*c3*D_xx(u):  du = (dx*D_t^T - nu*c3*D_xx^T)(gg) + dt*gg*D_x(u) + dt*D_x^T(gg*u)
struct VjpBurgers {
    static constexpr int FIN = 2, FOUT = 1;
    struct Params { Star lin, Dx, DxT; float dt; };      // lin = dx*Dt^T - nu*c3*Dxx^T
    static __device__ __forceinline__ void eval(const Nbr (&n)[2], const Params &p, float4 (&r)[1])
    {
        const Nbr gu = mul_nbr(n[0], n[1]);
        r[0] = apply<K_STAR7>(p.lin, n[0]) + p.dt * (mul4(n[0].c, apply<K_STAR7>(p.Dx, n[1])) + apply<K_STAR7>(p.DxT, gu));
    }
};

// ------------------------------------------------------------------ sum(m * r^2): two stages, fixed order, fp64
constexpr int SUMSQ_WAVES = 4;

// Stage 1: a wave per row of the [B*T*X, Y] view (rows dealt round-robin over the grid's waves), a lane per quad; every
// lane adds its squares in fp64 in the order it meets them, the workgroup's 256 lane sums are added by a fixed tree in LDS.
__global__ void __launch_bounds__(64 *SUMSQ_WAVES) sumsq_partial_kernel(const float *r, long long sB, long long sT, long long sX,
                                                                        int T, int X, int Y, long long rows, int crop,
                                                                        double *partial)
{
    __shared__ double red[64 * SUMSQ_WAVES];
    const int lane = threadIdx.x, wv = threadIdx.y;
    const bool cT = crop & CROP_T, cX = crop & CROP_X, cY = crop & CROP_Y;
    double acc = 0.0;
    for (long long row = (long long)blockIdx.x * SUMSQ_WAVES + wv; row < rows; row += (long long)gridDim.x * SUMSQ_WAVES) {
        const int x = (int)(row % X);
        const long long bt = row / X;
        const int t = (int)(bt % T);
        const long long b = bt / T;
        if ((cT && (t < 1 || t > T - 2)) || (cX && (x < 1 || x > X - 2))) continue;       // (wave-uniform)
        const float *p = r + b * sB + (long long)t * sT + (long long)x * sX;
        for (int y = 4 * lane; y < Y; y += 256) {
            float4 v = f4(0.f);
            if (y + 3 < Y) {
                v = ldg4(p + y);
            } else {
                v.x = p[y];
                if (y + 1 < Y) v.y = p[y + 1];
                if (y + 2 < Y) v.z = p[y + 2];
            }
            if (cY) {
                if (y < 1 || y > Y - 2) v.x = 0.f;                       // (a select: a NaN outside the crop is not summed)
                if (y + 1 > Y - 2) v.y = 0.f;
                if (y + 2 > Y - 2) v.z = 0.f;
                if (y + 3 > Y - 2) v.w = 0.f;
            }
            acc += ((double)v.x * (double)v.x + (double)v.y * (double)v.y) + ((double)v.z * (double)v.z + (double)v.w * (double)v.w);
        }
    }
    const int tid = wv * 64 + lane;
    red[tid] = acc;
    __syncthreads();
    for (int s = 32 * SUMSQ_WAVES; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = red[0];
}

// Stage 2: one workgroup adds the partials (each thread its strided share, in order; then the same fixed tree)
__global__ void __launch_bounds__(256) sumsq_final_kernel(const double *partial, int n, double *out)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n; i += 256) acc += partial[i];
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) *out = red[0];
}

}  // namespace

extern "C" {

int pre_vjp_abi_version(void) { return PRE_VJP_ABI_VERSION; }

int pre_vjp_stencil3d_f32(const pre_field_t *g, const pre_out_t *out, const float *tap_w, const int32_t *tap_off, int ntaps,
                          float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                          void *stream)
{
    if (ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    const pre_field_t *fs[1] = {g};
    const pre_out_t *os[1] = {out};
    VGeom vg;
    int rc = prepare_vjp(vg, fs, 1, os, 1, B, T, X, Y, crop_of(flags, false), host_scale, dev_scale);
    if (rc) return rc;
    Star s;
    if (!star_of_taps(tap_w, tap_off, ntaps, &s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    VjpLinear1::Params p{mirrored(s)};
    vg.tfree = !has_t(s);
    return launch_vjp<VjpLinear1>(vg, p, as_stream(stream));
}

int pre_vjp_stencil2d_f32(const float *g, const int64_t g_strides[3], float *out, const int64_t out_strides[3],
                          const float *tap_w, const int32_t *tap_off, int ntaps, float host_scale, const float *dev_scale,
                          int64_t B, int64_t T, int64_t X, int flags, void *stream)
{
    if (!g || !g_strides || !out || !out_strides || ntaps < 0 || (ntaps > 0 && (!tap_w || !tap_off))) return PRE_E_NULL;
    if (ntaps > 343) return PRE_E_SHAPE;
    // [B,T,X] with taps (dt,dx)  ==  [1,B,T,X] with taps (0,dt,dx)
    int32_t off3[3 * 343];
    for (int i = 0; i < ntaps; ++i) {
        off3[3 * i] = 0;
        off3[3 * i + 1] = tap_off[2 * i];
        off3[3 * i + 2] = tap_off[2 * i + 1];
    }
    pre_field_t fg{g, 0, g_strides[0], g_strides[1], g_strides[2]};
    pre_out_t o{out, 0, out_strides[0], out_strides[1], out_strides[2]};
    const pre_field_t *fs[1] = {&fg};
    const pre_out_t *os[1] = {&o};
    VGeom vg;
    int rc = prepare_vjp(vg, fs, 1, os, 1, 1, B, T, X, crop_of(flags, true), host_scale, dev_scale);
    if (rc) return rc;
    Star s;
    if (!star_of_taps(tap_w, off3, ntaps, &s, &rc)) return rc ? rc : PRE_E_UNSUPPORTED;
    VjpLinear1::Params p{mirrored(s)};
    vg.tfree = 1;
    return launch_vjp<VjpLinear1>(vg, p, as_stream(stream));
}

int pre_vjp_linear2_f32(const pre_field_t *g, const pre_out_t out[2], const float *K_a, const float *K_b, float ratio,
                        float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                        void *stream)
{
    if (!out || !K_a || !K_b) return PRE_E_NULL;
    const pre_field_t *fs[1] = {g};
    const pre_out_t *os[2] = {&out[0], &out[1]};
    VGeom vg;
    int rc = prepare_vjp(vg, fs, 1, os, 2, B, T, X, Y, crop_of(flags, false), host_scale, dev_scale);
    if (rc) return rc;
    Star a, b;
    if (!star_from_dense27(K_a, &a) || !star_from_dense27(K_b, &b)) return PRE_E_UNSUPPORTED;
    const Star zero{0, 0, 0, 0, 0, 0, 0};
    VjpLinear2::Params p{mirrored(a), combine((double)ratio, mirrored(b), 0.0, zero)};
    vg.tfree = !has_t(a) && !has_t(b);
    return launch_vjp<VjpLinear2>(vg, p, as_stream(stream));
}

int pre_vjp_burgers_f32(const float *g, const int64_t g_strides[3], const float *u, const int64_t u_strides[3], float *du,
                        const int64_t du_strides[3], const float *K_t, const float *K_x, const float *K_xx, float dx, float dt,
                        float nu, float c3, float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X,
                        int flags, void *stream)
{
    if (!g || !g_strides || !u || !u_strides || !du || !du_strides || !K_t || !K_x || !K_xx) return PRE_E_NULL;
    // [B,T,X] -> [1,B,T,X]; 3x3 kernel (a over Nt, b over Nx) -> dense27 index (1, a, b), as pre_residual_burgers_f32
    pre_field_t fg{g, 0, g_strides[0], g_strides[1], g_strides[2]}, fu{u, 0, u_strides[0], u_strides[1], u_strides[2]};
    pre_out_t o{du, 0, du_strides[0], du_strides[1], du_strides[2]};
    const pre_field_t *fs[2] = {&fg, &fu};
    const pre_out_t *os[1] = {&o};
    VGeom vg;
    int rc = prepare_vjp(vg, fs, 2, os, 1, 1, B, T, X, crop_of(flags, true), host_scale, dev_scale);
    if (rc) return rc;
    float d27[3][27] = {};
    const float *k9[3] = {K_t, K_x, K_xx};
    for (int op = 0; op < 3; ++op)
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) d27[op][(1 * 3 + i) * 3 + c] = k9[op][i * 3 + c];
    Star Dt, Dx, Dxx;
    if (!star_from_dense27(d27[0], &Dt) || !star_from_dense27(d27[1], &Dx) || !star_from_dense27(d27[2], &Dxx))
        return PRE_E_UNSUPPORTED;
    VjpBurgers::Params p;
    p.lin = combine((double)dx, mirrored(Dt), -((double)nu * (double)c3), mirrored(Dxx));
    p.Dx = Dx;
    p.DxT = mirrored(Dx);
    p.dt = dt;
    vg.tfree = 1;
    return launch_vjp<VjpBurgers>(vg, p, as_stream(stream));
}

int pre_vjp_ns_momentum_f32(const pre_field_t *g, const pre_field_t uv[2], const pre_out_t out[3], const float *K_t,
                            const float *K_x, const float *K_y, const float *K_xx_yy, float dt, float dx, float dy, float nu,
                            float host_scale, const float *dev_scale, int64_t B, int64_t T, int64_t X, int64_t Y, int flags,
                            void *stream)
{
    if (!uv || !out || !K_t || !K_x || !K_y || !K_xx_yy) return PRE_E_NULL;
    const pre_field_t *fs[3] = {g, &uv[0], &uv[1]};
    const pre_out_t *os[3] = {&out[0], &out[1], &out[2]};
    VGeom vg;
    int rc = prepare_vjp(vg, fs, 3, os, 3, B, T, X, Y, crop_of(flags, false), host_scale, dev_scale);
    if (rc) return rc;
    Star Dt, Dx, Dy, L;
    if (!star_from_dense27(K_t, &Dt) || !star_from_dense27(K_x, &Dx) || !star_from_dense27(K_y, &Dy) ||
        !star_from_dense27(K_xx_yy, &L))
        return PRE_E_UNSUPPORTED;
    const double a = (double)dx * dy, b = (double)dt * dy, c = (double)dt * dx, n = (double)nu * dt;
    VjpNSMomentum::Params p;
    p.lin = combine(a, mirrored(Dt), -n, mirrored(L));
    p.pT = combine(b, mirrored(Dx), c, mirrored(Dy));
    p.Dx = Dx; p.Dy = Dy;
    p.DxT = mirrored(Dx); p.DyT = mirrored(Dy);
    p.b = (float)b; p.c = (float)c;
    vg.tfree = !has_t(Dt) && !has_t(Dx) && !has_t(Dy) && !has_t(L);
    return launch_vjp<VjpNSMomentum>(vg, p, as_stream(stream));
}

int pre_vjp_sumsq_f32(const pre_field_t *r, int64_t B, int64_t T, int64_t X, int64_t Y, int flags, double *workspace,
                      double *out, void *stream)
{
    if (!r || !r->ptr || !workspace || !out || B <= 0 || T <= 0 || X <= 0 || Y <= 0) return PRE_E_NULL;
    if (B > 0x7fffffff || T > 0x7fffffff || X > 0x7fffffff || Y > 0x7fffffff - 8) return PRE_E_SHAPE;
    if (r->sY != 1) return PRE_E_UNSUPPORTED;
    const long long rows = (long long)B * T * X;
    // the grid is a function of the shape alone: the same view is always summed in the same order
    const long long want = (rows + SUMSQ_WAVES - 1) / SUMSQ_WAVES;
    const int blocks = (int)(want < PRE_VJP_SUMSQ_WORKSPACE ? want : PRE_VJP_SUMSQ_WORKSPACE);
    int crop = 0;
    if (flags & PRE_VJP_CROP) crop = (flags & PRE_VJP_VIEW3D) ? (CROP_X | CROP_Y) : (CROP_T | CROP_X | CROP_Y);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3((unsigned)blocks), dim3(64, SUMSQ_WAVES), 0, st, r->ptr, (long long)r->sB,
                       (long long)r->sT, (long long)r->sX, (int)T, (int)X, (int)Y, rows, crop, workspace);
    PRE_LAUNCH_CHECK();
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, st, workspace, blocks, out);
    PRE_LAUNCH_CHECK();
    return PRE_OK;
}

}  // extern "C"
