// f64_rate.hip -- the rate at which this device's vector unit issues uncontracted f64 multiplies and adds, the yardstick of
// tools/source_bench.py's arithmetic floor.
//   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off tools/f64_rate.hip -o tools/f64_rate && tools/f64_rate
// Every thread runs `iters` iterations of 16 independent x = x * a + b (one v_mul_f64 and one v_add_f64 each: built without
// contraction, like the library); 8 workgroups of 256 threads per compute unit (8 waves per SIMD in flight); timed by device events
// around the launch, the best of 5 after a warm-up.  Prints one line: f64 operations per second, the compute units, the clock.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define HIPC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

__global__ void __launch_bounds__(256) k_rate(double* out, int iters, double a, double b)
{
    double x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = (double)(threadIdx.x + i) * 1e-3;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int i = 0; i < 16; i++) x[i] = x[i] * a + b;
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 16; i++) s += x[i];
    if (s == 12345.678) out[0] = s;                     // (keeps the loop alive; never true for these inputs in practice, and out has room)
}

int main()
{
    hipDeviceProp_t prop;
    HIPC(hipGetDeviceProperties(&prop, 0));
    const int groups = prop.multiProcessorCount * 8, iters = 4096;
    double* out; HIPC(hipMalloc((void**)&out, sizeof(double)));
    hipEvent_t e0, e1; HIPC(hipEventCreate(&e0)); HIPC(hipEventCreate(&e1));
    float best = 1e30f;
    for (int rep = 0; rep < 6; rep++) {
        HIPC(hipEventRecord(e0, 0));
        k_rate<<<groups, 256, 0, 0>>>(out, iters, 0.999999, 1e-7);
        HIPC(hipEventRecord(e1, 0));
        HIPC(hipEventSynchronize(e1));
        float ms; HIPC(hipEventElapsedTime(&ms, e0, e1));
        if (rep && ms < best) best = ms;
    }
    const double ops = 2.0 * 16.0 * iters * 256.0 * groups;
    printf("%.6e f64_ops_per_s %d compute_units %d kHz %.4f ms\n", ops / (best * 1e-3), prop.multiProcessorCount, prop.clockRate, best);
    HIPC(hipFree(out));
    return 0;
}
