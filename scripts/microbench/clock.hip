// What is the shader clock under a latency-bound launch, and what does a dependent fp64 instruction cost?  One wavefront per CU
// runs a loop of s_nop 15 and, in a second kernel, a chain of dependent v_fma_f64 (measured: 2.62 ns = 6.3 cycles per link -- the
// floor of every single-wavefront recursion in the engines: 5.8 cycles per instruction in the factorisation sweep); wall time from s_memrealtime (100 MHz).  build: hipcc --offload-arch=gfx950 -O2
// What the factorisation sweep's pivot chain can hide (profiles/fact_pipe_ab.txt), one wavefront alone on its SIMD again: v_fma_f64 with
// 1, 2, 4, 8 independent accumulator chains (the issue cost once the dependency is out of the way), a chain of v_rcp_f64 each with its
// three refinement FMAs (csrc/mpc_ipm.h fast_rcp), and an LDS ds_write_b64 -> ds_read_b64 round trip inside the wavefront.
#include <hip/hip_runtime.h>
#include <cstdio>
__global__ void nops(long long *out, int iters)
{
    const long long t0 = wall_clock64();
    for (int i = 0; i < iters; i++) {
        asm volatile("s_nop 15\ns_nop 15\ns_nop 15\ns_nop 15\ns_nop 15\ns_nop 15\ns_nop 15\ns_nop 15" ::: "memory");
    }
    const long long t1 = wall_clock64();
    if (threadIdx.x == 0) out[blockIdx.x] = t1 - t0;
}
__global__ void fmas(long long *out, double *sink, int iters, double a, double b)
{
    double x = threadIdx.x;
    const long long t0 = wall_clock64();
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int j = 0; j < 16; j++) x = __builtin_fma(x, a, b);
    }
    const long long t1 = wall_clock64();
    if (threadIdx.x == 0) out[blockIdx.x] = t1 - t0;
    sink[blockIdx.x * blockDim.x + threadIdx.x] = x;
}
template <int C>
__global__ void fmas_ind(long long *out, double *sink, int iters, double a, double b)
{
    double x[C];
#pragma unroll
    for (int c = 0; c < C; c++) x[c] = threadIdx.x + c;
    const long long t0 = wall_clock64();
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int j = 0; j < 16 / C; j++)
#pragma unroll
            for (int c = 0; c < C; c++) x[c] = __builtin_fma(x[c], a, b);
    }
    const long long t1 = wall_clock64();
    if (threadIdx.x == 0) out[blockIdx.x] = t1 - t0;
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < C; c++) s += x[c];
    sink[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void rcps(long long *out, double *sink, int iters, double d0)
{
    double d = d0 + threadIdx.x;
    const long long t0 = wall_clock64();
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int j = 0; j < 8; j++) {       // fast_rcp: v_rcp_f64, e = fma(-d, x, 1), fma(x, fma(e, e, e), x); the next link inverts the result
            const double x = __builtin_amdgcn_rcp(d);
            const double e = __builtin_fma(-d, x, 1.0);
            d = __builtin_fma(x, __builtin_fma(e, e, e), x);
        }
    }
    const long long t1 = wall_clock64();
    if (threadIdx.x == 0) out[blockIdx.x] = t1 - t0;
    sink[blockIdx.x * blockDim.x + threadIdx.x] = d;
}
__global__ void lds_trip(long long *out, double *sink, int iters)
{
    __shared__ double buf[64];
    double v = threadIdx.x;
    const int other = threadIdx.x ^ 1;      // the neighbour's slot: the value has to come back from LDS
    const long long t0 = wall_clock64();
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            buf[threadIdx.x] = v;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // (the engines' wave-local phase boundary, mpc_devexec.h wave_fence)
            __builtin_amdgcn_wave_barrier();
            v = buf[other];
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    const long long t1 = wall_clock64();
    if (threadIdx.x == 0) out[blockIdx.x] = t1 - t0;
    sink[blockIdx.x * blockDim.x + threadIdx.x] = v;
}
template <int C>
static void run_ind(int blocks, long long *d, long long *h, double *sink, double cyc_ns)
{
    const int it = 1000000;
    fmas_ind<C><<<blocks, 64>>>(d, sink, it, 0.999999, 1e-9);
    hipDeviceSynchronize();
    hipMemcpy(h, d, blocks * 8, hipMemcpyDeviceToHost);
    const double ns = h[0] * 10.0 / ((double)it * 16);
    printf("v_fma_f64, %d independent chains, %3d wavefronts: %.2f ns = %.2f cycles per fma\n", C, blocks, ns, ns / cyc_ns);
}
int main()
{
    long long *d, h[256];
    double *sink;
    hipMalloc(&d, 256 * 8);
    hipMalloc(&sink, 256 * 256 * 8);
    for (int rep = 0; rep < 3; rep++) {
        for (int blocks : {1, 256}) {
            const int it = 2000000;
            nops<<<blocks, 64>>>(d, it);
            hipDeviceSynchronize();
            hipMemcpy(h, d, blocks * 8, hipMemcpyDeviceToHost);
            // (s_nop 15 holds the wavefront for 16 QUAD cycles + its own issue: 68 cycles -- 28.5 ns here = 2.39 GHz, the clock
            // GRBM_GUI_ACTIVE / 8 XCDs / kernel time gives for the real kernels as well)
            printf("s_nop 15, %3d wavefronts: %.2f ns each\n", blocks, h[0] * 10.0 / ((double)it * 8));
            const double cyc_ns = h[0] * 10.0 / ((double)it * 8) / 68.0;      // one shader cycle, from the line above
            const int itf = 1000000;
            fmas<<<blocks, 64>>>(d, sink, itf, 0.999999, 1e-9);
            hipDeviceSynchronize();
            hipMemcpy(h, d, blocks * 8, hipMemcpyDeviceToHost);
            printf("dependent v_fma_f64 chain, %3d wavefronts: %.2f ns per fma\n", blocks, h[0] * 10.0 / ((double)itf * 16));
            if (rep == 2) {
                run_ind<1>(blocks, d, h, sink, cyc_ns); run_ind<2>(blocks, d, h, sink, cyc_ns);
                run_ind<4>(blocks, d, h, sink, cyc_ns); run_ind<8>(blocks, d, h, sink, cyc_ns);
                const int itr = 500000;
                rcps<<<blocks, 64>>>(d, sink, itr, 1.5);
                hipDeviceSynchronize();
                hipMemcpy(h, d, blocks * 8, hipMemcpyDeviceToHost);
                double ns = h[0] * 10.0 / ((double)itr * 8);
                printf("dependent v_rcp_f64 + 3 refinement fma, %3d wavefronts: %.2f ns = %.2f cycles per link\n", blocks, ns, ns / cyc_ns);
                lds_trip<<<blocks, 64>>>(d, sink, itr);
                hipDeviceSynchronize();
                hipMemcpy(h, d, blocks * 8, hipMemcpyDeviceToHost);
                ns = h[0] * 10.0 / ((double)itr * 8);
                printf("LDS ds_write_b64 -> ds_read_b64 round trip, %3d wavefronts: %.2f ns = %.2f cycles\n", blocks, ns, ns / cyc_ns);
            }
        }
    }
    return 0;
}
