// kernels_warp.hip — the exact grid warp of a dense, row-major n x n plane of u16 (the alteration source into one image of the input
// buffer: musica_alter_warp) or u8 (one reference slot into another: musica_sim_warp_reference): a backward warp out[x] = in[x + d(x)]
// by a displacement field given on a control grid of spacing kWarpGrid = 64 pixels in units of 1 / kWarpUnit = 1 / 256 pixel, every
// component within +-kWarpMaxShift = 4096 (16 pixels). Pixel (x, y) sits at grid coordinate (x + o, y + o), 0 <= o < 64. harness.warp
// states, in integers, `>>` the arithmetic shift (a floor):
//   X = x + o,  cx = X >> 6,  fx = X & 63                                                     (Y, cy, fy likewise)
//   S_c = (64 - fy) ((64 - fx) d[cy, cx] + fx d[cy, cx + 1]) + fy ((64 - fx) d[cy + 1, cx] + fx d[cy + 1, cx + 1])       |S_c| <= 2^24
//   s_c = (S_c + 2048) >> 12                                                                  c = 0: dx, 1: dy
//   ix = x + (s_0 >> 8),  wx = s_0 & 255,  x0 = clamp(ix),  x1 = clamp(ix + 1)                (iy, wy, y0, y1 likewise; clamp to 0 .. n - 1)
//   out[y, x] = ((256 - wy) ((256 - wx) in[y0, x0] + wx in[y0, x1]) + wy ((256 - wx) in[y1, x0] + wx in[y1, x1]) + 32768) >> 16
// ONE rounding of the field, ONE of the image sum, halves up; the sum is at most 65535 * 65536 + 32768 < 2^32: every intermediate is an
// exact i32 or u32. The weights of S_c are convex and (4096 d + 2048) >> 12 = d, so s_c lies between the smallest and the largest of the
// four nodes of its cell.
//
// k_warp<T>: a workgroup of 256 threads owns one 64 x 64 tile of the output; one instantiation per type.
//   nodes    with an origin a tile spans at most 2 x 2 cells, so 3 x 3 nodes. A node travels as one u32, dx in the low half and dy in the
//            high one; its index depends on the workgroup alone, so the nine loads are the same in every lane (scalar loads). Indices past
//            the m x m array are clamped into it; such a node is used by no pixel of the plane.
//   window   the tile's displacements lie between the minimum and the maximum of the nodes its pixels use (convexity, above), per
//            component: the source window is columns clamp(x0 + (min_0 >> 8)) .. clamp(x0 + tw - 1 + (max_0 >> 8) + 1), rows likewise,
//            at most 63 + 16 + 1 + 16 + 1 = 97 = kWarpWin pixels a side, staged into LDS as u16 once. One pixel per lane and trip,
//            consecutive lanes on consecutive pixels of a window row. The trips are unrolled in two passes, loads into registers and
//            then the LDS writes, so that all of a thread's loads are in flight together; the loads read coordinates clamped into the
//            window (so inside the plane), and a trip that lies wholly below the window's last row is skipped by every lane alike.
//   sample   a thread owns 16 consecutive output rows of one column; consecutive lanes take consecutive columns and a wavefront one
//            row at a time, so cy and fy are the same in every lane and cx, fx fixed down a thread's run. The three node rows are
//            folded along x once per thread, H_r = (64 - fx) d[r, cx] + fx d[r, cx + 1]; per pixel S = (64 - fy) H_cy + fy H_(cy + 1),
//            the cell boundary inside a tile taken from Y >> 6 per row and X >> 6 per lane. The four source pixels are read from the
//            window at clamp(ix), clamp(ix + 1), ... minus the window's origin: the clamp is the plane's, and the window holds every
//            such index because its bounds are the same clamp of the extreme displacements. Neighbouring lanes read neighbouring u16 of
//            one or two window rows; the pitch is an odd number of dwords. Lanes and rows past a ragged tile's edge compute the tile's
//            last column or row again and store nothing;
//   store    one pixel per lane, consecutive lanes on consecutive pixels of a row, bounds-checked against the plane.
// 19 KB of LDS. Pixels are read and written as single T elements, so a plane needs no more than its element's alignment (image 1 of a
// batch with odd N^2 starts on a 2-byte boundary only). Nothing outside the two planes and the m x m nodes is read, nothing outside
// `out` written; the planes must not overlap.
#include "study_device.h"

namespace musica {

constexpr int kWarpThreads = 256;
constexpr int kWarpRun = 16;                                              // outputs per thread
constexpr int kWarpReach = kWarpMaxShift / kWarpUnit;                     // whole pixels of the largest displacement: 16
constexpr int kWarpWin = kSimTile - 1 + 2 * (kWarpReach + 1) ;            // largest side of a tile's source window: 97
constexpr int kWarpPitch = (((kWarpWin + 1) / 2) | 1) * 2;                // its LDS pitch in pixels: 49 dwords
constexpr int kWarpTrips = (kWarpWin * kWarpWin + kWarpThreads - 1) / kWarpThreads;   // staging trips of a thread
static_assert(kWarpGrid == kSimTile && kWarpGrid == 64, "X >> 6 and X & 63 are the cell and the offset; a tile spans at most 2 x 2 cells");
static_assert(kWarpUnit == 256, "s >> 8 and s & 255 are the whole and the fractional displacement");
static_assert(kWarpMaxShift % kWarpUnit == 0 && kWarpGrid * kWarpGrid * kWarpMaxShift <= (1 << 24), "|S_c| <= 2^24 and the reach is whole pixels");
static_assert(kWarpPitch >= kWarpWin && (kWarpPitch / 2) % 2 == 1, "the pitch holds a window row in an odd number of dwords");
static_assert(kSimTile * kSimTile == kWarpThreads * kWarpRun && kWarpThreads / kSimTile * kWarpRun == kSimTile, "a thread per column and run of rows of the tile");

template <typename T>
__global__ __launch_bounds__(kWarpThreads) void k_warp(const T* __restrict__ src, T* __restrict__ out, int n, const uint32_t* __restrict__ nodes, int m,
                                                       int o) {
    __shared__ uint16_t win[kWarpWin * kWarpPitch];
    const int tiles = (n + kSimTile - 1) / kSimTile;
    const TileGeom t = tile_geom(blockIdx.x, tiles, n, n);
    // the tile's first cell and the last node offset its pixels use along each axis (1: one cell, 2: two)
    const int cx0 = (t.x0 + o) >> 6, cy0 = (t.y0 + o) >> 6;
    const int ex = ((t.x0 + t.tw - 1 + o) >> 6) - cx0 + 1, ey = ((t.y0 + t.th - 1 + o) >> 6) - cy0 + 1;
    int d[3][3][2], lo[2] = {kWarpMaxShift, kWarpMaxShift}, hi[2] = {-kWarpMaxShift, -kWarpMaxShift};
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const uint32_t w = nodes[min(cy0 + j, m - 1) * m + min(cx0 + i, m - 1)];
            d[j][i][0] = (int)(int16_t)(w & 0xffffu);
            d[j][i][1] = (int)(int16_t)(w >> 16);
            if (j <= ey && i <= ex) {
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    lo[c] = min(lo[c], d[j][i][c]);
                    hi[c] = max(hi[c], d[j][i][c]);
                }
            }
        }
    // the window: the plane's clamp of the extreme source indices, so 1 <= ww, wh <= kWarpWin (kWarpReach bounds lo and hi)
    const int wx0 = min(max(t.x0 + (max(lo[0], -kWarpMaxShift) >> 8), 0), n - 1), wy0 = min(max(t.y0 + (max(lo[1], -kWarpMaxShift) >> 8), 0), n - 1);
    const int ww = min(min(max(t.x0 + t.tw - 1 + (min(hi[0], kWarpMaxShift) >> 8) + 1, 0), n - 1) - wx0 + 1, kWarpWin);
    const int wh = min(min(max(t.y0 + t.th - 1 + (min(hi[1], kWarpMaxShift) >> 8) + 1, 0), n - 1) - wy0 + 1, kWarpWin);

    // A fixed trip count, unrolled, in two passes: every load of a thread is issued before the first one is waited for. The loads are
    // unconditional on coordinates clamped into the window (so inside the plane); what lies past the window is dropped at the write.
    // A staged pixel keeps a register of its own (u8 ones packed four to a register would each be waited for), and an address is the
    // window's origin, the same in every lane, plus a 32-bit offset (at most 96 rows of 16384 pixels).
    uint32_t staged[kWarpTrips];
    const T* const origin = src + ((size_t)wy0 * n + wx0);
#pragma unroll
    for (int k = 0; k < kWarpTrips; k++) {
        if (k * kWarpThreads >= wh * kWarpWin) break;   // the same in every lane: the trip starts below the window
        const int e = k * kWarpThreads + (int)threadIdx.x;
        const int wy = e / kWarpWin, wx = e - wy * kWarpWin;
        staged[k] = origin[(uint32_t)(min(wy, wh - 1) * n + min(wx, ww - 1))];
    }
#pragma unroll
    for (int k = 0; k < kWarpTrips; k++) {
        if (k * kWarpThreads >= wh * kWarpWin) break;
        const int e = k * kWarpThreads + (int)threadIdx.x;
        const int wy = e / kWarpWin, wx = e - wy * kWarpWin;
        if (wy < wh && wx < ww) win[wy * kWarpPitch + wx] = (uint16_t)staged[k];
    }
    __syncthreads();

    // Lanes and rows past a ragged tile's edge take the tile's last column / row: their cells, nodes and window indices are the tile's.
    const int lane_x = threadIdx.x % kSimTile, y = threadIdx.x / kSimTile * kWarpRun;
    const int x = t.x0 + min(lane_x, t.tw - 1);
    const int X = x + o, cx = (X >> 6) - cx0, fx = X & 63;   // cx: 0 or 1
    T* const corner = out + ((size_t)t.y0 * n + t.x0);   // the tile's first pixel: the same in every lane, the stores add 32-bit offsets
    int H[3][2];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int c = 0; c < 2; c++) H[j][c] = (64 - fx) * (cx ? d[j][1][c] : d[j][0][c]) + fx * (cx ? d[j][2][c] : d[j][1][c]);   // |H| <= 2^18
#pragma unroll
    for (int k = 0; k < kWarpRun; k++) {
        const int yy = t.y0 + min(y + k, t.th - 1);
        const int Y = yy + o, cy = (Y >> 6) - cy0, fy = Y & 63;   // the same in every lane of the wavefront; cy: 0 or 1
        const int s0 = ((64 - fy) * (cy ? H[1][0] : H[0][0]) + fy * (cy ? H[2][0] : H[1][0]) + 2048) >> 12;
        const int s1 = ((64 - fy) * (cy ? H[1][1] : H[0][1]) + fy * (cy ? H[2][1] : H[1][1]) + 2048) >> 12;
        const int ix = x + (s0 >> 8), iy = yy + (s1 >> 8);
        const uint32_t wx = (uint32_t)(s0 & 255), wy = (uint32_t)(s1 & 255);
        const int lx0 = min(max(ix, 0), n - 1) - wx0, lx1 = min(max(ix + 1, 0), n - 1) - wx0;
        const int r0 = (min(max(iy, 0), n - 1) - wy0) * kWarpPitch, r1 = (min(max(iy + 1, 0), n - 1) - wy0) * kWarpPitch;
        const uint32_t top = (256u - wx) * win[r0 + lx0] + wx * win[r0 + lx1];      // <= 65535 * 256
        const uint32_t bottom = (256u - wx) * win[r1 + lx0] + wx * win[r1 + lx1];
        const uint32_t s = (256u - wy) * top + wy * bottom + 32768u;
        if (lane_x < t.tw && y + k < t.th) corner[(uint32_t)((y + k) * n + lane_x)] = (T)(s >> 16);
    }
}

template <typename T>
static void launch_warp(hipStream_t st, const T* src, T* out, int n, const uint32_t* nodes, int m, int origin) {
    const unsigned tiles = (unsigned)((n + kSimTile - 1) / kSimTile);
    hipLaunchKernelGGL((k_warp<T>), dim3(tiles * tiles), dim3(kWarpThreads), 0, st, src, out, n, nodes, m, origin);
}

void launch_warp_u16(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const uint32_t* nodes, int m, int origin) {
    launch_warp<uint16_t>(st, src, out, n, nodes, m, origin);
}
void launch_warp_u8(hipStream_t st, const uint8_t* src, uint8_t* out, int n, const uint32_t* nodes, int m, int origin) {
    launch_warp<uint8_t>(st, src, out, n, nodes, m, origin);
}

}  // namespace musica
