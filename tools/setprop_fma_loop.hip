// A plain fp64 FMA loop: the device's fp64 vector FMA rate, measured beside tools/setprop_bench.py's kernels in the same
// run.  Each thread runs 8 independent chains of `iters` dependent FMAs and stores one sum so nothing is eliminated.
#include <hip/hip_runtime.h>

__global__ void __launch_bounds__(256) fma_loop_kernel(double *out, int iters, double m)
{
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = threadIdx.x * 1e-3 + i;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = fma(v[i], m, 1e-7);
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v[i];
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = s;
}

extern "C" int fma_loop(double *out, int blocks, int iters, double m, void *stream)
{
    hipLaunchKernelGGL(fma_loop_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, iters, m);
    return (int)hipGetLastError();
}
