// transpose_gather.hip — the form kernels_symmetry.hip's LDS tiles replace, measured once and not part of the library: the transpose of
// an n x n u16 plane as a plain per-thread gather, the way k_alter gathers (kernels_alteration.hip). Every thread owns 8 consecutive
// output pixels and stores them with one 16-byte store; their 8 source pixels lie one row pitch apart, 2 bytes each.
// `pairs` source / destination planes are used in turn so that no launch finds its planes in the 256 MiB Infinity Cache.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 devtools/transpose_gather.hip -o devtools/transpose_gather
//   devtools/transpose_gather [n = 3072] [launches = 60] [pairs = 12]      (kernel times: run it under rocprofv3 --kernel-trace)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ __launch_bounds__(256) void k_transpose_gather(const uint16_t* __restrict__ src, uint16_t* __restrict__ out, int n) {
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (p0 >= (long long)n * n) return;   // n % 8 == 0: a thread's 8 pixels are in one row
    const int i = (int)(p0 / n), j = (int)(p0 - (long long)i * n);
    union {
        uint16_t px[8];
        uint4 v;
    } u;
#pragma unroll
    for (int e = 0; e < 8; e++) u.px[e] = src[(size_t)(j + e) * n + i];
    *reinterpret_cast<uint4*>(out + p0) = u.v;
}

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 3072, launches = argc > 2 ? atoi(argv[2]) : 60, pairs = argc > 3 ? atoi(argv[3]) : 12;
    if (n < 8 || n % 8 || n > 16384 || launches < 1 || pairs < 1 || pairs > 64) { fprintf(stderr, "need n %% 8 == 0 in [8, 16384], launches >= 1, 1 <= pairs <= 64\n"); return 2; }
    const size_t nn = (size_t)n * n;
    std::vector<uint16_t> h(nn), back(nn);
    for (size_t k = 0; k < nn; k++) h[k] = (uint16_t)(k * 2654435761u >> 13);
    std::vector<uint16_t*> src(pairs), dst(pairs);
    for (int k = 0; k < pairs; k++) {
        OK(hipMalloc(&src[k], nn * 2));
        OK(hipMalloc(&dst[k], nn * 2));
        OK(hipMemcpy(src[k], h.data(), nn * 2, hipMemcpyHostToDevice));
    }
    const unsigned blocks = (unsigned)((nn / 8 + 255) / 256);
    hipEvent_t a, b;
    OK(hipEventCreate(&a));
    OK(hipEventCreate(&b));
    std::vector<float> us;
    for (int l = 0; l < launches + pairs; l++) {   // the first round warms up
        const int k = l % pairs;
        OK(hipEventRecord(a, 0));
        hipLaunchKernelGGL(k_transpose_gather, dim3(blocks), dim3(256), 0, 0, src[k], dst[k], n);
        OK(hipEventRecord(b, 0));
        OK(hipEventSynchronize(b));
        float ms = 0.f;
        OK(hipEventElapsedTime(&ms, a, b));
        if (l >= pairs) us.push_back(ms * 1e3f);
    }
    OK(hipMemcpy(back.data(), dst[0], nn * 2, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++)
            if (back[(size_t)i * n + j] != h[(size_t)j * n + i]) { fprintf(stderr, "wrong pixel at (%d, %d)\n", i, j); return 1; }
    std::sort(us.begin(), us.end());
    printf("{\"n\": %d, \"launches\": %d, \"pairs\": %d, \"event_us_median\": %.2f, \"event_us_min\": %.2f, \"event_us_max\": %.2f}\n", n, launches, pairs,
           us[us.size() / 2], us.front(), us.back());
    for (int k = 0; k < pairs; k++) { (void)hipFree(src[k]); (void)hipFree(dst[k]); }
    return 0;
}
