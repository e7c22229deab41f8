// Dev tool: k_zoom<uint16_t> and k_zoom<uint8_t> (kernels_zoom.hip, compiled into this program) alone, timed with HIP events on
// full-range random planes: the launches rotate over `pairs` source / destination pairs so that, with enough of them, no launch finds
// its planes in the 256 MiB Infinity Cache (12 pairs x 37.7 MB for u16 at 3072^2); pairs = 1 is the cache-resident case, which is what
// devtools/copy_ceiling.hip measures with its single pair. Prints per zoom and type the back-to-back time per launch, the median of
// single launches between their own event pair, and the rate over the algorithmic bytes (1 + (q / p)^2) n^2 sizeof(T).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include devtools/zoom_probe.hip -o zoom_probe
//   ./zoom_probe [n = 3072] [pairs = 12] [rounds = 10]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <random>
#include <vector>

#include "../metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd/csrc/kernels_zoom.hip"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

static void launch(hipStream_t st, const uint16_t* s, uint16_t* d, int n, int p, int q) { musica::launch_zoom_u16(st, s, d, n, p, q); }
static void launch(hipStream_t st, const uint8_t* s, uint8_t* d, int n, int p, int q) { musica::launch_zoom_u8(st, s, d, n, p, q); }

template <typename T>
static void probe(const char* type, int n, int pairs, int rounds) {
    const size_t count = (size_t)n * n;
    std::vector<T> host(count);
    std::mt19937 gen(1);
    for (auto& v : host) v = (T)gen();
    std::vector<T*> src(pairs), dst(pairs);
    for (int k = 0; k < pairs; k++) {
        CK(hipMalloc(&src[k], count * sizeof(T)));
        CK(hipMalloc(&dst[k], count * sizeof(T)));
        CK(hipMemcpy(src[k], host.data(), count * sizeof(T), hipMemcpyHostToDevice));
    }
    hipStream_t st;
    CK(hipStreamCreate(&st));
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    const int zooms[2][2] = {{21, 20}, {2, 1}};
    for (const auto& z : zooms) {
        const int p = z[0], q = z[1];
        const double bytes = (1.0 + (double)q * q / ((double)p * p)) * (double)count * sizeof(T);
        for (int k = 0; k < pairs; k++) launch(st, src[k], dst[k], n, p, q);   // warm: the code object, every page
        CK(hipStreamSynchronize(st));
        CK(hipEventRecord(a, st));
        for (int i = 0; i < rounds * pairs; i++) launch(st, src[i % pairs], dst[i % pairs], n, p, q);
        CK(hipEventRecord(b, st));
        CK(hipEventSynchronize(b));
        CK(hipGetLastError());
        float ms;
        CK(hipEventElapsedTime(&ms, a, b));
        const double each = ms * 1e3 / (rounds * pairs);
        std::vector<float> t;
        for (int i = 0; i < rounds * pairs; i++) {
            CK(hipEventRecord(a, st));
            launch(st, src[i % pairs], dst[i % pairs], n, p, q);
            CK(hipEventRecord(b, st));
            CK(hipEventSynchronize(b));
            CK(hipEventElapsedTime(&ms, a, b));
            t.push_back(ms * 1e3f);
        }
        std::sort(t.begin(), t.end());
        const double med = t[t.size() / 2];
        printf("k_zoom<%s> n=%d zoom %d/%d pairs=%d: %.2f us/launch back-to-back (%.0f GB/s), one event pair per launch: median %.2f us "
               "(%.0f GB/s), min %.2f, max %.2f; %.1f MB algorithmic\n",
               type, n, p, q, pairs, each, bytes / (each * 1e-6) / 1e9, med, bytes / (med * 1e-6) / 1e9, t.front(), t.back(), bytes / 1e6);
    }
    for (int k = 0; k < pairs; k++) {
        CK(hipFree(src[k]));
        CK(hipFree(dst[k]));
    }
    CK(hipEventDestroy(a));
    CK(hipEventDestroy(b));
    CK(hipStreamDestroy(st));
}

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 3072;
    const int pairs = argc > 2 ? atoi(argv[2]) : 12;
    const int rounds = argc > 3 ? atoi(argv[3]) : 10;
    if (n < 1 || pairs < 1 || rounds < 1) return 2;
    probe<uint16_t>("uint16_t", n, pairs, rounds);
    probe<uint8_t>("uint8_t", n - 2 * MUSICA_OUT_MARGIN > 0 ? n - 2 * MUSICA_OUT_MARGIN : n, pairs, rounds);   // a reference slot's side
    return 0;
}
