// kernels_blur.hip — the exact binomial blur of a dense, row-major n x n plane of u16 (the alteration source into one image of the input
// buffer: musica_alter_blur) or u8 (one reference slot into another: musica_sim_blur_reference). With radius r (1 .. 8) and the
// weights w_k = C(2r, k), k = 0 .. 2r (their sum is 4^r), harness.binomial_blur states
//   out[y, x] = (sum_i sum_j w_i w_j in[clamp(y + i - r), clamp(x + j - r)] + 2^(4r - 1)) >> 4r
// with indices clamped to the plane (edge replicated), ONE rounding after the full 2-D sum, halves up. Every intermediate is an exact
// integer: a row sum of u16 data needs 16 + 2r <= 32 bits, the full sum 16 + 4r <= 48.
//
// k_blur<T, R>: a workgroup of 256 threads owns one 64 x 64 tile of the output.
//   stage    the clamped (64 + 2R)^2 source window into LDS as u16, so HBM sees each source pixel once per tile (halo: 1.56 x at R = 8);
//   rows     the row pass into an LDS plane of u32 sums, (64 + 2R) rows x 64 columns. A thread owns 16 consecutive outputs of one window
//            row and slides over its 16 + 2R pixels in registers (dword reads, two pixels each), folding w_k = w_{2R - k}; consecutive
//            lanes take consecutive rows, and both planes have an odd pitch in dwords, so neither the reads nor the writes collide on a
//            bank;
//   columns  a thread owns 16 consecutive output rows of one column and slides over its 16 + 2R row sums in registers; consecutive lanes
//            take consecutive columns. The accumulator is u32 where 8 sizeof(T) + 4R <= 32 and u64 (v_mad_u64_u32) otherwise;
//   store    one pixel per lane, consecutive lanes on consecutive pixels of a row, bounds-checked against the plane.
// 13.1 + 20.8 KB of LDS at R = 8: four workgroups per CU. Pixels are read and written as single T elements, so a plane needs no more
// than its element's alignment (image 1 of a batch with odd N^2 starts on a 2-byte boundary only). Nothing outside the two planes is
// read or written; the planes must not overlap.
#include <type_traits>

#include "kernels_common.h"
#include "launchers.h"

namespace musica {

constexpr int kBlurThreads = 256;
constexpr int kBlurTile = 64;
constexpr int kBlurRun = 16;   // outputs per thread and pass

__host__ __device__ constexpr uint32_t blur_weight(int r, int k) {   // C(2r, k): exact at every step, <= 12870
    uint32_t c = 1;
    for (int i = 0; i < k; i++) c = c * (uint32_t)(2 * r - i) / (uint32_t)(i + 1);
    return c;
}

template <typename T, int R>
__global__ __launch_bounds__(kBlurThreads) void k_blur(const T* __restrict__ src, T* __restrict__ out, int n) {
    constexpr int W = kBlurTile + 2 * R;              // side of the source window
    constexpr int SP = ((W / 2) | 1) * 2;             // its LDS pitch in pixels: an odd number of dwords
    constexpr int HP = kBlurTile + 1;                 // pitch of the row sums in dwords
    constexpr int GROUPS = kBlurTile / kBlurRun;      // runs per row (rows pass), per column (columns pass)
    constexpr int TAPS = kBlurRun + 2 * R;            // what one run reads
    typedef typename std::conditional<(8 * sizeof(T) + 4 * R <= 32), uint32_t, unsigned long long>::type Acc;
    __shared__ uint32_t win_words[W * SP / 2];
    __shared__ uint32_t sums[W * HP];
    uint16_t* win = reinterpret_cast<uint16_t*>(win_words);
    const int x0 = blockIdx.x * kBlurTile, y0 = blockIdx.y * kBlurTile;

    for (int p = threadIdx.x; p < W * W; p += kBlurThreads) {
        const int wy = p / W, wx = p - wy * W;
        const int gy = min(max(y0 - R + wy, 0), n - 1), gx = min(max(x0 - R + wx, 0), n - 1);
        win[wy * SP + wx] = (uint16_t)src[(size_t)gy * n + gx];
    }
    __syncthreads();

    for (int item = threadIdx.x; item < W * GROUPS; item += kBlurThreads) {
        const int g = item / W, wy = item - g * W;
        uint32_t px[TAPS];
#pragma unroll
        for (int d = 0; d < TAPS / 2; d++) {
            const uint32_t two = win_words[(wy * SP + g * kBlurRun) / 2 + d];
            px[2 * d] = two & 0xffffu;
            px[2 * d + 1] = two >> 16;
        }
#pragma unroll
        for (int k = 0; k < kBlurRun; k++) {
            uint32_t s = blur_weight(R, R) * px[k + R];
#pragma unroll
            for (int j = 0; j < R; j++) s += blur_weight(R, j) * (px[k + j] + px[k + 2 * R - j]);
            sums[wy * HP + g * kBlurRun + k] = s;
        }
    }
    __syncthreads();

    const int x = threadIdx.x % kBlurTile, g = threadIdx.x / kBlurTile;
    uint32_t h[TAPS];
#pragma unroll
    for (int i = 0; i < TAPS; i++) h[i] = sums[(g * kBlurRun + i) * HP + x];
    const int gx = x0 + x;
#pragma unroll
    for (int k = 0; k < kBlurRun; k++) {
        Acc s = (Acc)1 << (4 * R - 1);
#pragma unroll
        for (int i = 0; i <= 2 * R; i++) s += (Acc)blur_weight(R, i) * h[k + i];
        const int gy = y0 + g * kBlurRun + k;
        if (gx < n && gy < n) out[(size_t)gy * n + gx] = (T)(s >> (4 * R));
    }
}

template <typename T, int R>
static void launch_blur_r(hipStream_t st, const T* src, T* out, int n) {
    const unsigned tiles = (unsigned)((n + kBlurTile - 1) / kBlurTile);
    hipLaunchKernelGGL((k_blur<T, R>), dim3(tiles, tiles), dim3(kBlurThreads), 0, st, src, out, n);
}

template <typename T>
static void launch_blur(hipStream_t st, const T* src, T* out, int n, int radius) {
    static_assert(kBlurMaxRadius == 8, "one instantiation per radius");
    switch (radius) {
        case 1: launch_blur_r<T, 1>(st, src, out, n); break;
        case 2: launch_blur_r<T, 2>(st, src, out, n); break;
        case 3: launch_blur_r<T, 3>(st, src, out, n); break;
        case 4: launch_blur_r<T, 4>(st, src, out, n); break;
        case 5: launch_blur_r<T, 5>(st, src, out, n); break;
        case 6: launch_blur_r<T, 6>(st, src, out, n); break;
        case 7: launch_blur_r<T, 7>(st, src, out, n); break;
        case 8: launch_blur_r<T, 8>(st, src, out, n); break;
        default: break;
    }
}

void launch_blur_u16(hipStream_t st, const uint16_t* src, uint16_t* out, int n, int radius) { launch_blur<uint16_t>(st, src, out, n, radius); }
void launch_blur_u8(hipStream_t st, const uint8_t* src, uint8_t* out, int n, int radius) { launch_blur<uint8_t>(st, src, out, n, radius); }

}  // namespace musica
