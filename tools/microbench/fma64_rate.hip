// The f64 multiply-add rate of the whole chip on gfx950: a bare loop of v_fma_f64 on 8 independent accumulators per thread (no
// instruction waits for the one before it), operands in registers, no memory traffic; workgroups of 256 threads, `--waves` wavefronts
// per SIMD resident.  Wall time between two events around the launch: f64 multiply-adds per second, the yardstick the convolve pass of
// the programme bank is held against (tools/bench_program_convolve.py, DESIGN.md section 10 "Convolve").
// hipcc --offload-arch=gfx950 -O3 fma64_rate.hip -o fma64_rate; ./fma64_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <string>
#include <vector>

constexpr int ITERS = 2048, UNROLL = 8, CHAINS = 8;

__global__ __launch_bounds__(256) void fma64_kernel(double seed, double scale, double* sink) {
    double d[CHAINS];
    for (int c = 0; c < CHAINS; ++c) d[c] = seed + c + threadIdx.x;
    for (int i = 0; i < ITERS; ++i) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
            for (int c = 0; c < CHAINS; ++c) d[c] = __builtin_fma(d[c], scale, 0.5);
        }
    }
    double acc = 0.0;
    for (int c = 0; c < CHAINS; ++c) acc += d[c];
    sink[(size_t)blockIdx.x * 256 + threadIdx.x] = acc;
}

int main(int argc, char** argv) {
    int waves = 2;  // per SIMD
    for (int i = 1; i + 1 < argc; i += 2)
        if (std::string(argv[i]) == "--waves") waves = std::atoi(argv[i + 1]);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
    const int blocks = prop.multiProcessorCount * waves * 8;  // 8 rounds of a full chip: 4 SIMDs per CU, one workgroup is 4 wavefronts
    double* sink;
    if (hipMalloc(&sink, (size_t)blocks * 256 * sizeof(double)) != hipSuccess) return 1;
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    std::vector<float> ms;
    for (int rep = 0; rep < 12; ++rep) {
        (void)hipEventRecord(a, 0);
        hipLaunchKernelGGL(fma64_kernel, dim3(blocks), dim3(256), 0, 0, 1.0, 0.9999999, sink);
        (void)hipEventRecord(b, 0);
        if (hipEventSynchronize(b) != hipSuccess) return 1;
        float t = 0.0f;
        (void)hipEventElapsedTime(&t, a, b);
        if (rep >= 2) ms.push_back(t);  // (two warm-up launches)
    }
    std::sort(ms.begin(), ms.end());
    const double fmas = (double)blocks * 256 * ITERS * UNROLL * CHAINS;
    const double median = ms[ms.size() / 2];
    printf("fma64_rate: %d CUs, %d workgroups of 256, %.3g f64 multiply-adds per launch: median %.4f ms (min %.4f, max %.4f, %zu launches), "
           "%.2f T multiply-adds/s (%.2f TFLOP/s)\n",
           prop.multiProcessorCount, blocks, fmas, median, ms.front(), ms.back(), ms.size(), fmas / (median * 1e-3) / 1e12,
           2.0 * fmas / (median * 1e-3) / 1e12);
    (void)hipFree(sink);
    return 0;
}
