// FP64 issue rate on gfx950: vector fused multiply-add (v_fma_f64) against the matrix instruction v_mfma_f64_16x16x4_f64, for the
// K15 decision.  Every wave runs ITER rounds over 16 independent accumulator chains (FMA: 16 doubles per lane; MFMA:
// 4 accumulator tiles of 4 doubles per lane, 4 instructions per round unrolled 4 times); 4 waves per SIMD on every CU.
// Prints the median of 5 timed launches after one warm-up.
//   hipcc --offload-arch=gfx950 -O3 -o ub_f64_rate ub_f64_rate.hip && ./ub_f64_rate
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int ITER = 20000;

__global__ __launch_bounds__(256) void k_fma(double* out, double a, double b) {
    double acc[16];
    for (int i = 0; i < 16; ++i) acc[i] = threadIdx.x + i;
    for (int it = 0; it < ITER; ++it)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = fma(acc[i], a, b);
    double s = 0;
    for (int i = 0; i < 16; ++i) s += acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_mfma(double* out, double a, double b) {
    d4 acc[4];
    for (int i = 0; i < 4; ++i) acc[i] = d4{(double)threadIdx.x, 1.0, 2.0, (double)i};
    for (int it = 0; it < ITER; ++it)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    double s = 0;
    for (int i = 0; i < 4; ++i) s += acc[i].x + acc[i].y + acc[i].z + acc[i].w;
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <typename K>
static double median_ms(K kernel, double* d, int blocks) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    float t[5];
    for (int r = -1; r < 5; ++r) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, 0, d, 0.999999, 1e-9);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        if (r >= 0) hipEventElapsedTime(&t[r], e0, e1);
    }
    std::sort(t, t + 5);
    return t[2];
}

int main() {
    const int blocks = 256 * 4;                       // 4 workgroups of 4 waves per CU: 4 waves per SIMD
    double* d = nullptr;
    if (hipMalloc((void**)&d, (size_t)blocks * 256 * sizeof(double)) != hipSuccess) { printf("no device\n"); return 1; }
    const double tf = median_ms(k_fma, d, blocks), tm = median_ms(k_mfma, d, blocks);
    const double waves = (double)blocks * 4;
    const double flops_fma = waves * 64.0 * 16 * ITER * 2;                       // 2 flops per lane and instruction
    const double flops_mfma = waves * 16.0 * ITER * (2.0 * 16 * 16 * 4);         // 16 instructions per round, 2 m n k flops each
    printf("{\"fma_ms\": %.3f, \"fma_tflops\": %.2f, \"mfma_ms\": %.3f, \"mfma_tflops\": %.2f}\n", tf, flops_fma / tf / 1e9, tm,
           flops_mfma / tm / 1e9);
    hipFree(d);
    return 0;
}
