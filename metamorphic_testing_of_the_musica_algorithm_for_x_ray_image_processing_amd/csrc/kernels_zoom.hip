// kernels_zoom.hip — the exact rational zoom of a dense, row-major n x n plane of u16 (the alteration source into one image of the input
// buffer: musica_alter_zoom) or u8 (one reference slot into another: musica_sim_zoom_reference): magnification by p / q about the
// plane's centre, bilinear, in integers. With 1 <= q < p <= 32, gcd(p, q) = 1 and D = 2p, harness.zoom states for an output index x
//   n_x = (2x - (n - 1)) q + (n - 1) p   (>= 0; the source coordinate is n_x / D),   i_x = n_x div D,   f_x = n_x mod D,   g_x = D - f_x
//   out[y, x] = (g_y g_x in[i_y, i_x] + g_y f_x in[i_y, i_x+] + f_y g_x in[i_y+, i_x] + f_y f_x in[i_y+, i_x+] + D^2 / 2) div D^2
// with i+ = min(i + 1, n - 1): ONE rounding after the full 2-D sum, halves up. The weights sum to D^2 <= 4096 and the sum is at most
// 65535 * 4096 + 2048 < 2^32, so every intermediate is an exact u32. A zoom >= 1 about the centre reads only inside the plane: there is
// no fill value, and the clamp in i+ is met only where f = 0 and its weight with it.
//
// k_zoom<T>: a workgroup of 256 threads owns one 64 x 64 tile of the output; p and q are runtime values, one instantiation per type.
//   stage    the tile's source window into LDS as u16: rows i_y(y0) .. i_y+(last row of the tile), columns likewise, origin and extent
//            computed once per workgroup. Output steps are q / p < 1 source pixels, so i(x0 + 63) - i(x0) <= 63 and with i+ the window
//            never exceeds 65 <= kZoomWin pixels a side. One pixel per lane and trip, consecutive lanes on consecutive pixels of a
//            window row: HBM sees each source pixel once per tile. The trips are unrolled in two passes, loads into registers and then
//            the LDS writes, so that all of a thread's loads are in flight together;
//   sample   a thread owns 16 consecutive output rows of one column; consecutive lanes take consecutive columns, so a wavefront reads
//            a window row at non-decreasing columns (equal ones broadcast, the others lie on neighbouring banks) and the window's pitch
//            is an odd number of dwords, so that a column read would not stay on one bank either. (i_x, f_x) come from one division
//            per thread and the row pair is folded along x once per source row: top = g_x in[i_y, i_x] + f_x in[i_y, i_x+]. Down the
//            run f_y += 2q, and on f_y >= D: f_y -= D, i_y += 1, the bottom row becomes the top one and one new row is folded (at most
//            one carry per step, since 2q < D; the carry is the same in every lane of a wavefront). out = (g_y top + f_y bottom +
//            D^2 / 2) div D^2, the divisor uniform;
//   store    one pixel per lane, consecutive lanes on consecutive pixels of a row, bounds-checked against the plane.
// 8.7 KB of LDS, 68 VGPRs. Pixels are read and written as single T elements, so a plane needs no more than its element's alignment (image 1 of a
// batch with odd N^2 starts on a 2-byte boundary only). Nothing outside the two planes is read or written; the planes must not overlap.
#include "study_device.h"

namespace musica {

constexpr int kZoomThreads = 256;
constexpr int kZoomRun = 16;                          // outputs per thread
constexpr int kZoomWin = 66;                          // largest side of a tile's source window
constexpr int kZoomPitch = (((kZoomWin + 1) / 2) | 1) * 2;   // its LDS pitch in pixels: 33 dwords
constexpr int kZoomTrips = (kZoomWin * kZoomWin + kZoomThreads - 1) / kZoomThreads;   // staging trips of a thread
static_assert(kZoomPitch >= kZoomWin && (kZoomPitch / 2) % 2 == 1, "the pitch holds a window row in an odd number of dwords");
static_assert(kSimTile * kSimTile == kZoomThreads * kZoomRun, "a thread per column and run of rows of the tile");

// n_x of output index x: the source coordinate in units of 1 / (2p). x < 2^26 keeps it in an int.
__device__ __forceinline__ int zoom_num(int x, int n, int p, int q) { return (2 * x - (n - 1)) * q + (n - 1) * p; }

template <typename T>
__global__ __launch_bounds__(kZoomThreads) void k_zoom(const T* __restrict__ src, T* __restrict__ out, int n, int p, int q) {
    __shared__ uint16_t win[kZoomWin * kZoomPitch];
    const int tiles = (n + kSimTile - 1) / kSimTile;
    const TileGeom t = tile_geom(blockIdx.x, tiles, n, n);
    const int D = 2 * p;
    // the window: first source index of the tile's first output, i+ of its last one
    const int wx0 = zoom_num(t.x0, n, p, q) / D, wy0 = zoom_num(t.y0, n, p, q) / D;
    const int ww = min(min(zoom_num(t.x0 + t.tw - 1, n, p, q) / D + 1, n - 1) - wx0 + 1, kZoomWin);
    const int wh = min(min(zoom_num(t.y0 + t.th - 1, n, p, q) / D + 1, n - 1) - wy0 + 1, kZoomWin);

    // A fixed trip count, unrolled, in two passes: every load of a thread is issued before the first one is waited for. The loads are
    // unconditional on coordinates clamped into the window (so inside the plane); what lies past the window is dropped at the write.
    T staged[kZoomTrips];
#pragma unroll
    for (int k = 0; k < kZoomTrips; k++) {
        const int e = k * kZoomThreads + (int)threadIdx.x;
        const int wy = e / kZoomWin, wx = e - wy * kZoomWin;
        staged[k] = src[(size_t)(wy0 + min(wy, wh - 1)) * n + (wx0 + min(wx, ww - 1))];
    }
#pragma unroll
    for (int k = 0; k < kZoomTrips; k++) {
        const int e = k * kZoomThreads + (int)threadIdx.x;
        const int wy = e / kZoomWin, wx = e - wy * kZoomWin;
        if (wy < wh && wx < ww) win[wy * kZoomPitch + wx] = (uint16_t)staged[k];
    }
    __syncthreads();

    // Lanes and rows past a ragged tile's edge compute on clamped window indices and store nothing.
    const int x = threadIdx.x % kSimTile, y = threadIdx.x / kSimTile * kZoomRun;
    const int nx = zoom_num(t.x0 + x, n, p, q), ny = zoom_num(t.y0 + y, n, p, q);
    const int ix = nx / D, iy = ny / D;
    const uint32_t fx = (uint32_t)(nx - ix * D), gx = (uint32_t)D - fx;
    const int lx = min(ix - wx0, ww - 1), lx1 = min(lx + 1, ww - 1);
    auto folded = [&](int ly) { return gx * win[ly * kZoomPitch + lx] + fx * win[ly * kZoomPitch + lx1]; };   // <= 65535 D

    uint32_t fy = (uint32_t)(ny - iy * D);
    int ly = min(iy - wy0, wh - 1);
    uint32_t top = folded(ly), bottom = folded(min(ly + 1, wh - 1));
    const uint32_t d2 = (uint32_t)(D * D);
#pragma unroll
    for (int k = 0; k < kZoomRun; k++) {
        const uint32_t s = ((uint32_t)D - fy) * top + fy * bottom + d2 / 2;
        if (x < t.tw && y + k < t.th) out[(size_t)(t.y0 + y + k) * n + (t.x0 + x)] = (T)(s / d2);
        fy += 2u * (uint32_t)q;
        if (fy >= (uint32_t)D) {
            fy -= (uint32_t)D;
            ly = min(ly + 1, wh - 1);
            top = bottom;
            bottom = folded(min(ly + 1, wh - 1));
        }
    }
}

template <typename T>
static void launch_zoom(hipStream_t st, const T* src, T* out, int n, int p, int q) {
    const unsigned tiles = (unsigned)((n + kSimTile - 1) / kSimTile);
    hipLaunchKernelGGL((k_zoom<T>), dim3(tiles * tiles), dim3(kZoomThreads), 0, st, src, out, n, p, q);
}

void launch_zoom_u16(hipStream_t st, const uint16_t* src, uint16_t* out, int n, int p, int q) { launch_zoom<uint16_t>(st, src, out, n, p, q); }
void launch_zoom_u8(hipStream_t st, const uint8_t* src, uint8_t* out, int n, int p, int q) { launch_zoom<uint8_t>(st, src, out, n, p, q); }

}  // namespace musica
