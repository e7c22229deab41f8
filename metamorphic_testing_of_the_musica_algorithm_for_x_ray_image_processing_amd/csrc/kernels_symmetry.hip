// kernels_symmetry.hip — the eight symmetries of the square (the dihedral group D4) of a dense, row-major n x n plane of u16 (the
// alteration source into one image of the input buffer: musica_alter, MUSICA_ALTER_SYMMETRY) or u8 (one reference slot into another:
// musica_sim_transform_reference). Element e is np.rot90(x if e < 4 else x.T, e & 3) (harness.apply_symmetry); output pixel (i, j) is
//   0: in[i, j]   1: in[j, n-1-i]   2: in[n-1-i, n-1-j]   3: in[n-1-j, i]   4: in[j, i]   5: in[n-1-i, j]   6: in[n-1-j, n-1-i]   7: in[i, n-1-j]
// Every element is a permutation: no fill, no resampling, every pixel read once and written once.
//
// Elements 0, 2, 5, 7 keep rows as rows (k_sym_rows): a thread moves one W-byte word of a row, W = 16 where the row length in bytes and
// both planes are multiples of 16, else 4, else one pixel; the mirrored elements take the mirrored word and reverse its pixels in
// registers, so loads and stores are both contiguous over the wavefront.
//
// Elements 1, 3, 4, 6 swap the axes (k_sym_swap): a workgroup of 256 threads owns one 64 x 64 tile of the OUTPUT. It reads the source
// tile with consecutive lanes on consecutive source dwords of a row (128-byte runs for u16, 64-byte runs for u8), scatters the pixels
// of each dword into an LDS image of the output tile (the transposition and the two possible reversals happen in this index), and
// after the barrier reads LDS rows as dwords and stores them with consecutive lanes on consecutive output dwords. The LDS rows are
// padded by one dword (pitch 33 dwords for u16, 17 for u8): the dword reads and the scatter's dword-aligned neighbours then fall on
// different banks instead of one. Tiles that cross the plane's edge, and planes whose rows are not a whole number of dwords (odd
// sides; a u8 side that is not a multiple of 4) or that do not start on a dword, take the same path pixel by pixel, every access
// bounds-checked. Nothing outside the two planes is read or written.
#include "kernels_common.h"
#include "launchers.h"

namespace musica {

constexpr int kSymThreads = 256;
constexpr int kSymTile = 64;

typedef uint32_t __attribute__((may_alias)) sym_u32;   // a dword of pixels, read or written through a pixel pointer

template <int W> struct SymWord;
template <> struct SymWord<16> { typedef uint4 type; };
template <> struct SymWord<4> { typedef uint32_t type; };
template <> struct SymWord<2> { typedef uint16_t type; };
template <> struct SymWord<1> { typedef uint8_t type; };

// out[i, j] = src[FLIP_I ? n-1-i : i, FLIP_J ? n-1-j : j], one W-byte word per thread; n * sizeof(T) % W == 0 and both planes W-aligned
template <typename T, int W, bool FLIP_I, bool FLIP_J>
__global__ __launch_bounds__(kSymThreads) void k_sym_rows(const T* __restrict__ src, T* __restrict__ out, int n) {
    typedef typename SymWord<W>::type __attribute__((may_alias)) Word;
    constexpr int V = W / (int)sizeof(T);
    const uint32_t words = (uint32_t)n / V;   // per row
    const uint32_t t = blockIdx.x * kSymThreads + threadIdx.x;
    if (t >= (uint32_t)n * words) return;
    const uint32_t i = t / words, c = t - i * words;
    const uint32_t si = FLIP_I ? (uint32_t)n - 1 - i : i, sc = FLIP_J ? words - 1 - c : c;
    union {
        typename SymWord<W>::type w;
        T px[V];
    } a, b;
    a.w = *reinterpret_cast<const Word*>(src + (size_t)si * n + (size_t)sc * V);
    if (FLIP_J) {
#pragma unroll
        for (int k = 0; k < V; k++) b.px[k] = a.px[V - 1 - k];
    } else {
        b.w = a.w;
    }
    *reinterpret_cast<Word*>(out + (size_t)i * n + (size_t)c * V) = b.w;
}

// out[i, j] = src[FLIP_R ? n-1-j : j, FLIP_C ? n-1-i : i]; grid (ceil(n / 64), ceil(n / 64)), block (x, y) owns output rows 64 y .. and
// columns 64 x ... wide: rows are whole dwords and both planes start on one, so tiles inside the plane move dwords.
template <typename T, bool FLIP_R, bool FLIP_C>
__global__ __launch_bounds__(kSymThreads) void k_sym_swap(const T* __restrict__ src, T* __restrict__ out, int n, int wide) {
    constexpr int K = 4 / (int)sizeof(T);                  // pixels per dword
    constexpr int RD = kSymTile / K;                       // dwords per tile row
    constexpr int PD = RD + 1;                             // LDS pitch in dwords
    constexpr int PP = PD * K;                             // ... in pixels
    constexpr int PER = kSymTile * RD / kSymThreads;       // dwords per thread
    constexpr int SHIFT = 8 * (int)sizeof(T);
    __shared__ uint32_t lds[kSymTile * PD];                // the output tile: pixel (y, x) at y * PP + x
    T* tile = reinterpret_cast<T*>(lds);
    const int i0 = blockIdx.y * kSymTile, j0 = blockIdx.x * kSymTile;
    // the source tile's origin; LDS pixel (y, x) = source pixel (sr0 + a, sc0 + b) with x = FLIP_R ? 63 - a : a, y = FLIP_C ? 63 - b : b
    const int sr0 = FLIP_R ? n - kSymTile - j0 : j0;
    const int sc0 = FLIP_C ? n - kSymTile - i0 : i0;
    if (wide && i0 + kSymTile <= n && j0 + kSymTile <= n) {   // then 0 <= sr0, sc0 and the source tile is inside too
        uint32_t w[PER];
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int d = threadIdx.x + k * kSymThreads, a = d / RD, dc = d % RD;
            w[k] = *reinterpret_cast<const sym_u32*>(src + (size_t)(sr0 + a) * n + sc0 + dc * K);
        }
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int d = threadIdx.x + k * kSymThreads, a = d / RD, dc = d % RD;
            const int x = FLIP_R ? kSymTile - 1 - a : a;
#pragma unroll
            for (int q = 0; q < K; q++) {
                const int b = dc * K + q, y = FLIP_C ? kSymTile - 1 - b : b;
                tile[y * PP + x] = (T)(w[k] >> (SHIFT * q));
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int d = threadIdx.x + k * kSymThreads, y = d / RD, dc = d % RD;
            *reinterpret_cast<sym_u32*>(out + (size_t)(i0 + y) * n + j0 + dc * K) = reinterpret_cast<const sym_u32*>(tile)[y * PD + dc];
        }
        return;
    }
    for (int p = threadIdx.x; p < kSymTile * kSymTile; p += kSymThreads) {
        const int a = p / kSymTile, b = p % kSymTile, r = sr0 + a, c = sc0 + b;
        if (r < 0 || r >= n || c < 0 || c >= n) continue;
        const int x = FLIP_R ? kSymTile - 1 - a : a, y = FLIP_C ? kSymTile - 1 - b : b;
        tile[y * PP + x] = src[(size_t)r * n + c];
    }
    __syncthreads();
    for (int p = threadIdx.x; p < kSymTile * kSymTile; p += kSymThreads) {
        const int y = p / kSymTile, x = p % kSymTile;
        if (i0 + y < n && j0 + x < n) out[(size_t)(i0 + y) * n + j0 + x] = tile[y * PP + x];   // its source pixel is inside: loaded above
    }
}

static bool aligned_to(const void* p, const void* q, size_t row_bytes, size_t w) {
    return reinterpret_cast<uintptr_t>(p) % w == 0 && reinterpret_cast<uintptr_t>(q) % w == 0 && row_bytes % w == 0;
}

template <typename T, bool FLIP_I, bool FLIP_J>
static void launch_rows(hipStream_t st, const T* src, T* out, int n) {
    const size_t row_bytes = (size_t)n * sizeof(T);
    const int w = aligned_to(src, out, row_bytes, 16) ? 16 : (aligned_to(src, out, row_bytes, 4) ? 4 : (int)sizeof(T));
    const unsigned long long words = (unsigned long long)n * (row_bytes / w);
    const dim3 grid((unsigned)((words + kSymThreads - 1) / kSymThreads)), block(kSymThreads);
    if (w == 16) hipLaunchKernelGGL((k_sym_rows<T, 16, FLIP_I, FLIP_J>), grid, block, 0, st, src, out, n);
    else if (w == 4) hipLaunchKernelGGL((k_sym_rows<T, 4, FLIP_I, FLIP_J>), grid, block, 0, st, src, out, n);
    else hipLaunchKernelGGL((k_sym_rows<T, (int)sizeof(T), FLIP_I, FLIP_J>), grid, block, 0, st, src, out, n);
}

template <typename T, bool FLIP_R, bool FLIP_C>
static void launch_swap(hipStream_t st, const T* src, T* out, int n) {
    const unsigned tiles = (unsigned)((n + kSymTile - 1) / kSymTile);
    const int wide = aligned_to(src, out, (size_t)n * sizeof(T), 4);
    hipLaunchKernelGGL((k_sym_swap<T, FLIP_R, FLIP_C>), dim3(tiles, tiles), dim3(kSymThreads), 0, st, src, out, n, wide);
}

template <typename T>
static void launch_symmetry(hipStream_t st, const T* src, T* out, int n, int element) {
    switch (element) {
        case 0: launch_rows<T, false, false>(st, src, out, n); break;
        case 1: launch_swap<T, false, true>(st, src, out, n); break;
        case 2: launch_rows<T, true, true>(st, src, out, n); break;
        case 3: launch_swap<T, true, false>(st, src, out, n); break;
        case 4: launch_swap<T, false, false>(st, src, out, n); break;
        case 5: launch_rows<T, true, false>(st, src, out, n); break;
        case 6: launch_swap<T, true, true>(st, src, out, n); break;
        case 7: launch_rows<T, false, true>(st, src, out, n); break;
        default: break;
    }
}

void launch_symmetry_u16(hipStream_t st, const uint16_t* src, uint16_t* out, int n, int element) { launch_symmetry<uint16_t>(st, src, out, n, element); }
void launch_symmetry_u8(hipStream_t st, const uint8_t* src, uint8_t* out, int n, int element) { launch_symmetry<uint8_t>(st, src, out, n, element); }

}  // namespace musica
