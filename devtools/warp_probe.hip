// Dev tool: k_warp<uint16_t> and k_warp<uint8_t> (kernels_warp.hip) beside k_zoom (kernels_zoom.hip), both compiled into this program,
// alone, timed with HIP events on full-range random planes exactly as devtools/zoom_probe.hip times k_zoom: the launches rotate over
// `pairs` source / destination pairs so that, with enough of them, no launch finds its planes in the 256 MiB Infinity Cache; pairs = 1
// is the cache-resident case. Prints per field (zero: the window is the tile and one pixel; a bulge of 6 pixels; random nodes over
// the whole +-16 pixels: the widest windows) and type the back-to-back time per launch, the median of single launches between their
// own event pair, and the rate over the algorithmic bytes 2 n^2 sizeof(T); then the same for k_zoom at 21 / 20.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include devtools/warp_probe.hip -o warp_probe
//   ./warp_probe [n = 2048] [pairs = 12] [rounds = 10]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <functional>
#include <random>
#include <vector>

#include "../metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd/csrc/kernels_warp.hip"
#include "../metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd/csrc/kernels_zoom.hip"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

static void warp(hipStream_t st, const uint16_t* s, uint16_t* d, int n, const uint32_t* f, int m, int o) { musica::launch_warp_u16(st, s, d, n, f, m, o); }
static void warp(hipStream_t st, const uint8_t* s, uint8_t* d, int n, const uint32_t* f, int m, int o) { musica::launch_warp_u8(st, s, d, n, f, m, o); }
static void zoom(hipStream_t st, const uint16_t* s, uint16_t* d, int n, int p, int q) { musica::launch_zoom_u16(st, s, d, n, p, q); }
static void zoom(hipStream_t st, const uint8_t* s, uint8_t* d, int n, int p, int q) { musica::launch_zoom_u8(st, s, d, n, p, q); }

static uint32_t node(int dx, int dy) { return (uint32_t)(uint16_t)(int16_t)dx | (uint32_t)(uint16_t)(int16_t)dy << 16; }

template <typename T>
static void probe(const char* type, int n, int origin, int pairs, int rounds) {
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
    const int m = ((n - 1 + origin) >> 6) + 2;
    std::vector<uint32_t> fields[3];
    for (auto& f : fields) f.assign((size_t)m * m, 0u);
    for (int j = 0; j < m; j++)
        for (int i = 0; i < m; i++) {
            const double u = 2.0 * i / (m - 1) - 1.0, v = 2.0 * j / (m - 1) - 1.0, w = (1.0 - u * u) * (1.0 - v * v);
            fields[1][(size_t)j * m + i] = node((int)(4096.0 * u * w), (int)(4096.0 * v * w));
            fields[2][(size_t)j * m + i] = node((int)(gen() % 8193u) - 4096, (int)(gen() % 8193u) - 4096);
        }
    uint32_t* d_nodes;
    CK(hipMalloc(&d_nodes, (size_t)m * m * sizeof(uint32_t)));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    const char* names[4] = {"k_warp zero field", "k_warp bulge", "k_warp random +-16 px", "k_zoom 21/20"};
    for (int which = 0; which < 4; which++) {
        if (which < 3) CK(hipMemcpy(d_nodes, fields[which].data(), (size_t)m * m * sizeof(uint32_t), hipMemcpyHostToDevice));
        std::function<void(int)> launch = [&](int k) {
            if (which < 3) warp(st, src[k], dst[k], n, d_nodes, m, origin);
            else zoom(st, src[k], dst[k], n, 21, 20);
        };
        const double bytes = (which < 3 ? 2.0 : 1.0 + 400.0 / 441.0) * (double)count * sizeof(T);
        for (int k = 0; k < pairs; k++) launch(k);   // warm: the code object, every page
        CK(hipStreamSynchronize(st));
        CK(hipEventRecord(a, st));
        for (int i = 0; i < rounds * pairs; i++) launch(i % pairs);
        CK(hipEventRecord(b, st));
        CK(hipEventSynchronize(b));
        CK(hipGetLastError());
        float ms;
        CK(hipEventElapsedTime(&ms, a, b));
        const double each = ms * 1e3 / (rounds * pairs);
        std::vector<float> t;
        for (int i = 0; i < rounds * pairs; i++) {
            CK(hipEventRecord(a, st));
            launch(i % pairs);
            CK(hipEventRecord(b, st));
            CK(hipEventSynchronize(b));
            CK(hipEventElapsedTime(&ms, a, b));
            t.push_back(ms * 1e3f);
        }
        std::sort(t.begin(), t.end());
        const double med = t[t.size() / 2];
        printf("%s <%s> n=%d origin=%d pairs=%d: %.2f us/launch back-to-back (%.0f GB/s), one event pair per launch: median %.2f us "
               "(%.0f GB/s), min %.2f, max %.2f; %.1f MB algorithmic\n",
               names[which], type, n, origin, pairs, each, bytes / (each * 1e-6) / 1e9, med, bytes / (med * 1e-6) / 1e9, t.front(), t.back(), bytes / 1e6);
    }
    CK(hipFree(d_nodes));
    for (int k = 0; k < pairs; k++) {
        CK(hipFree(src[k]));
        CK(hipFree(dst[k]));
    }
    CK(hipEventDestroy(a));
    CK(hipEventDestroy(b));
    CK(hipStreamDestroy(st));
}

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 2048;
    const int pairs = argc > 2 ? atoi(argv[2]) : 12;
    const int rounds = argc > 3 ? atoi(argv[3]) : 10;
    if (n < 1 || n > 16384 || pairs < 1 || rounds < 1) return 2;
    probe<uint16_t>("uint16_t", n, 0, pairs, rounds);
    probe<uint8_t>("uint8_t", n - 2 * MUSICA_OUT_MARGIN > 0 ? n - 2 * MUSICA_OUT_MARGIN : n, MUSICA_OUT_MARGIN, pairs, rounds);   // a reference slot's side and origin
    return 0;
}
