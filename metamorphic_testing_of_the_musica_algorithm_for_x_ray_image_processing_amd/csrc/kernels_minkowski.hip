// kernels_minkowski.hip — the shape metric of the study (musica_sim_minkowski, include/musica.h; metrics.minkowski_statistics): the cell
// histograms from which the Minkowski functionals (area, perimeter, Euler characteristic) of every threshold set {v >= t} of a side
// follow. A side is a uint8 plane over the region, which is its own domain: side 0 the graded f32 plane of a batch image quantised with
// out_u8 while it is read (load_quant4: exactly what k_sim reads), side 1 a reference slot, side 2 their pixel-wise minimum. Per side
// eight 256-bin histograms [kind][value]: 0 the pixels; 1 / 2 / 3 the pixel edges between horizontal neighbours, between vertical
// neighbours and the pixel corners, the region's outline included, by the MAXIMUM of their incident pixels that exist (the closed
// cubical complex); 4 / 5 / 6 the interior ones by the MINIMUM of theirs (the open complex); 7 the 2 w + 2 h outline edges by their
// one pixel. No float arithmetic, no division, no scratch.
//
// k_minkowski: a query owns blockIdx.z; blockIdx.y is ONE side, which `groups` PERSISTENT workgroups of kStudyThreads threads share:
// workgroup g takes the 64 x 64 tiles g, g + groups, .. of the region (tile_geom).
//   stage    the tile with a halo of ONE pixel on the left and above, clipped to the region, as packed bytes in LDS
//            (stage_halo_window): tile pixel (tx, ty) is byte 16 + tx of window row ty + 1, so a thread's words are aligned. No
//            pixel outside the region (or the plane) is read: the other bytes of the window are 0, the neutral value of a maximum,
//            and a minimum that would use one is not counted (the run bounds below). Side 2 stages both planes and takes the
//            byte-wise minimum of the two windows once.
//   own      half-open: a pixel's tile owns its face, its left and its upper edge and its upper-left corner, so that a cell on a
//            tile seam is counted exactly once, by the tile right of or below the seam; where the pixel lies in the region's last
//            column or row, also the outline cells beyond it (the right edge and the upper-right corner; the lower edge and the
//            lower-left corner; the lower-right corner of the last pixel).
//   count    thread t takes the 16 consecutive pixels 16 q .. 16 q + 15 (q = t & 3) of tile row t / 4: one ds_read_b128 of its row
//            and one of the row above; the left neighbours are the same words turned by one byte with the word before them
//            (v_alignbyte_b32, shifted_words). The maxima and minima of four packed bytes are two v_pk_max_u16 / v_pk_min_u16 on the
//            even and the odd bytes (the granulometry's idiom). Which k of a run count is two integers a kind: lo <= k < hi.
//   add      into the workgroup's u32 counters in LDS, kept over all its tiles (THE WIDTH RULE), see CONTENTION.
//   flush    once a workgroup, behind its last tile: the replicas of a counter are summed and every NON-ZERO counter goes to the
//            query's table, which the caller zeroes on the stream, with one u32 global atomic: one a touched counter, never one a cell.
// THE WIDTH RULE. The counters are u32, not packed u16: nothing wraps, so there is no flush rule. A region's side is at most 16364, so
// a kind has at most 16365^2 < 2^29 cells; a workgroup's counter, a replica of it and the global word are each at most that.
// CONTENTION is the whole cost. On a flat area every cell of a kind wants one counter, and the LDS serialises equal addresses of one
// instruction. The two means of kernels_cooccurrence.hip, both measured here:
//   runs      a lane walks its 16 cells of a kind in order and adds a run of equal values with ONE ds_add_u32 of the run's length: on
//             a flat area 1 atomic for 16 cells, on noise 16 for 16 plus a compare and a branch a cell. At 3072^2, one / four
//             queries: 164 / 481 us against 266 / 820 without runs on a processed phantom, 140 / 400 against 421 / 1416 on a constant
//             plane, 144 / 406 against 149 / 382 on random planes: 6 % slower there with four queries.
//   replicas  kMinkowskiCopies copies of every counter, the copy of lane t being t mod copies and the copies of a counter
//             neighbouring words: lanes that want one counter hit different banks. 8 KiB a copy, which is occupancy: on the
//             phantom one / two / four copies take 194 / 164 / 149 us with one query and 571 / 481 / 582 with four. Two are shipped.
// Integer sums commute: the tables are exact and byte-identical from call to call and for any number of workgroups
// (MUSICA_MINKOWSKI_GROUPS, musica_study.hip).
// MUSICA_MINKOWSKI_GLOBAL_ATOMICS (a devtools/build_variant.sh build, for the A/B of DESIGN.md section 4; not shipped) replaces the LDS
// counters with one global atomic per cell; MUSICA_MINKOWSKI_NO_RUNS adds every cell on its own and MUSICA_MINKOWSKI_ONE_COPY keeps one
// copy of a counter (likewise).
#include "study_device.h"

namespace musica {

constexpr int kMinkPad = 16;                                  // window bytes left of the tile's first column: the halo pixel is byte 15
constexpr int kMinkWinRows = kSimTile + 1;                    // the halo row above, then the tile's
constexpr int kMinkWords = (kMinkPad + kSimTile) / 4;         // 20 staged words a row
constexpr int kMinkPitch = kMinkWords;                        // a multiple of 4 for ds_read_b128
constexpr int kMinkBins = kMinkowskiKinds * 256;
#ifdef MUSICA_MINKOWSKI_ONE_COPY
constexpr int kMinkowskiCopies = 1;
#else
constexpr int kMinkowskiCopies = 2;   // four are 10 % faster with one query on a processed plane and 21 - 45 % slower with four (LDS, occupancy)
#endif
static_assert(kSimTile == 64 && kStudyThreads == 256, "a thread takes 16 pixels of a row: four lanes a row, 64 rows");
static_assert(kMinkPad % 16 == 0 && kMinkPitch % 4 == 0, "aligned runs; the word before a run exists");
static_assert((kMinkowskiCopies & (kMinkowskiCopies - 1)) == 0, "the copy of a lane is a mask of its number");

enum MinkKind { kFace = 0, kAnyH, kAnyV, kAnyX, kAllH, kAllV, kAllX, kOutline };

typedef unsigned short MinkU16x2 __attribute__((ext_vector_type(2)));

// The maximum (minimum) of every byte of x and y: the even and the odd bytes as two u16 pairs
template <bool MAX>
__device__ __forceinline__ uint32_t mink_op(uint32_t x, uint32_t y) {
    const MinkU16x2 xe = __builtin_bit_cast(MinkU16x2, x & 0x00FF00FFu), ye = __builtin_bit_cast(MinkU16x2, y & 0x00FF00FFu);
    const MinkU16x2 xo = __builtin_bit_cast(MinkU16x2, (x >> 8) & 0x00FF00FFu), yo = __builtin_bit_cast(MinkU16x2, (y >> 8) & 0x00FF00FFu);
    const MinkU16x2 e = MAX ? __builtin_elementwise_max(xe, ye) : __builtin_elementwise_min(xe, ye);
    const MinkU16x2 o = MAX ? __builtin_elementwise_max(xo, yo) : __builtin_elementwise_min(xo, yo);
    return __builtin_bit_cast(uint32_t, e) | (__builtin_bit_cast(uint32_t, o) << 8);
}
template <bool MAX>
__device__ __forceinline__ void mink_op4(const uint32_t (&x)[4], const uint32_t (&y)[4], uint32_t (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = mink_op<MAX>(x[i], y[i]);
}

// One cell of value v into a kind's counters
__device__ __forceinline__ void mink_one(uint32_t* __restrict__ tab, GlobalU32* __restrict__ out, uint32_t v, int copy) {
#ifdef MUSICA_MINKOWSKI_GLOBAL_ATOMICS
    atomicAdd((uint32_t*)(out + v), 1u);
#else
    atomicAdd(&tab[v * kMinkowskiCopies + copy], 1u);
#endif
}

// The cells lo <= k < hi of a run, the value of cell k being byte k of V, into a kind's counters
__device__ __forceinline__ void mink_run(uint32_t* __restrict__ tab, GlobalU32* __restrict__ out, const uint32_t (&V)[4], int lo, int hi, int copy) {
    uint32_t cur = 0u, n = 0u;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t v = (V[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        if (k < lo || k >= hi) continue;
#if defined(MUSICA_MINKOWSKI_GLOBAL_ATOMICS) || defined(MUSICA_MINKOWSKI_NO_RUNS)
        mink_one(tab, out, v, copy);
#else
        if (n && v != cur) {
            atomicAdd(&tab[cur * kMinkowskiCopies + copy], n);
            n = 0u;
        }
        cur = v;
        n++;
#endif
    }
    if (n) atomicAdd(&tab[cur * kMinkowskiCopies + copy], n);
}

__global__ __launch_bounds__(kStudyThreads) void k_minkowski(const MinkowskiQueryDev* __restrict__ qs, uint32_t* __restrict__ tables) {
    constexpr int R = kMinkowskiCopies;
    __shared__ __attribute__((aligned(16))) uint32_t win[kMinkWinRows * kMinkPitch];
    __shared__ __attribute__((aligned(16))) uint32_t other[kMinkWinRows * kMinkPitch];   // side 2: the reference's window
#ifdef MUSICA_MINKOWSKI_GLOBAL_ATOMICS
    uint32_t* const tab = nullptr;
#else
    __shared__ uint32_t tab[kMinkBins * R];
#endif
    const MinkowskiQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.groups) return;   // whole workgroup: the grid is sized for the query with the most groups
    const int t = threadIdx.x, row = t >> 2, c0 = 16 * (t & 3), copy = t & (R - 1);
    const int side = (int)blockIdx.y;          // < kMinkowskiSides
    GlobalU32* const out = (GlobalU32*)tables + q.table + (size_t)side * kMinkBins;   // table [side][kind][value]
#ifndef MUSICA_MINKOWSKI_GLOBAL_ATOMICS
    for (int i = t; i < kMinkBins * R; i += kStudyThreads) tab[i] = 0u;
#endif
    const uint32_t* const mine = win + (row + 1) * kMinkPitch + (kMinkPad + c0) / 4;   // the run's pixels; word >= 4
    const uint32_t* const above = mine - kMinkPitch;                                    // the row above them: window row >= 0
    const uint8_t* const bytes = (const uint8_t*)win + (row + 1) * kMinkPitch * 4 + kMinkPad + c0;
    const auto same = [](uint32_t w) { return w; };
    const auto kind = [&](int k) { return tab + k * 256 * R; };
    const auto dest = [&](int k) { return out + k * 256; };

    const int tiles = q.tiles_x * q.tiles_y;
    for (int tile = blockIdx.x; tile < tiles; tile += q.groups) {
        const TileGeom g = tile_geom(tile, q.tiles_x, q.w, q.h);
        __syncthreads();   // the last tile's window is read; the first time: the counters are cleared
        const int x_lo = max(g.x0 - 1, 0), x_hi = g.x0 + g.tw, y_lo = max(g.y0 - 1, 0), y_hi = g.y0 + g.th;   // inside the region
        if (side != 1) stage_halo_window((const GlobalF32*)q.a, q.a_pitch, g.x0 - kMinkPad, g.y0 - 1, x_lo, x_hi, y_lo, y_hi, win, kMinkPitch, kMinkWords, kMinkWinRows, same);
        if (side != 0) stage_halo_window((const GlobalU8*)q.b, q.b_pitch, g.x0 - kMinkPad, g.y0 - 1, x_lo, x_hi, y_lo, y_hi, side == 1 ? win : other, kMinkPitch, kMinkWords, kMinkWinRows, same);
        if (side == 2) {
            __syncthreads();
            for (int i = t; i < kMinkWinRows * kMinkPitch; i += kStudyThreads) win[i] = mink_op<false>(win[i], other[i]);
        }
        __syncthreads();
        const int n = min(16, g.tw - c0);   // the run's pixels k < n lie in the tile
        if (row < g.th && n > 0) {          // the tile's rows; a ragged last tile has fewer
            const int x = g.x0 + c0, y = g.y0 + row;   // the region's pixel of k = 0
            const int lo = x == 0 ? 1 : 0;              // the left neighbour of pixel k exists: k >= lo
            uint32_t P[4], U[4], L[4], UL[4], H[4], V[4], X[4];
            const uint4 p = *reinterpret_cast<const uint4*>(mine), u = *reinterpret_cast<const uint4*>(above);
            P[0] = p.x, P[1] = p.y, P[2] = p.z, P[3] = p.w;
            U[0] = u.x, U[1] = u.y, U[2] = u.z, U[3] = u.w;
            shifted_words(mine[-1], P[0], P[1], P[2], P[3], 3u, L);      // byte k: pixel k - 1
            shifted_words(above[-1], U[0], U[1], U[2], U[3], 3u, UL);
            mink_run(kind(kFace), dest(kFace), P, 0, n, copy);
            mink_op4<true>(P, L, H);
            mink_run(kind(kAnyH), dest(kAnyH), H, 0, n, copy);           // the left edge; a pixel that does not exist is 0
            mink_op4<true>(P, U, V);
            mink_run(kind(kAnyV), dest(kAnyV), V, 0, n, copy);           // the upper edge
            mink_op4<true>(U, UL, X);
            mink_op4<true>(X, H, X);
            mink_run(kind(kAnyX), dest(kAnyX), X, 0, n, copy);           // the upper-left corner
            mink_op4<false>(P, L, X);
            mink_run(kind(kAllH), dest(kAllH), X, lo, n, copy);
            if (y > 0) {
                mink_op4<false>(P, U, V);
                mink_run(kind(kAllV), dest(kAllV), V, 0, n, copy);
                mink_op4<false>(U, UL, U);
                mink_op4<false>(X, U, X);
                mink_run(kind(kAllX), dest(kAllX), X, lo, n, copy);
            } else {
                mink_run(kind(kOutline), dest(kOutline), P, 0, n, copy);   // the region's upper outline
            }
            if (y == q.h - 1) {   // the region's last row: its lower outline, the lower edges and the lower-left corners
                mink_run(kind(kOutline), dest(kOutline), P, 0, n, copy);
                mink_run(kind(kAnyV), dest(kAnyV), P, 0, n, copy);
                mink_run(kind(kAnyX), dest(kAnyX), H, 0, n, copy);
            }
            if (x == 0) mink_one(kind(kOutline), dest(kOutline), bytes[0], copy);   // the region's left outline
            const int last = q.w - 1 - x;
            if (last < n) {       // the region's last column is this run's pixel `last`: 0 <= last because n <= w - x
                const uint32_t pv = bytes[last], uv = bytes[last - kMinkPitch * 4];   // the pixel and the one above it (0 where y is 0)
                mink_one(kind(kOutline), dest(kOutline), pv, copy);
                mink_one(kind(kAnyH), dest(kAnyH), pv, copy);                        // the right edge
                mink_one(kind(kAnyX), dest(kAnyX), max(pv, uv), copy);               // the upper-right corner
                if (y == q.h - 1) mink_one(kind(kAnyX), dest(kAnyX), pv, copy);      // the lower-right corner
            }
        }
    }
#ifndef MUSICA_MINKOWSKI_GLOBAL_ATOMICS
    __syncthreads();
    for (int i = t; i < kMinkBins; i += kStudyThreads) {
        uint32_t sum = 0u;
#pragma unroll
        for (int r = 0; r < R; r++) sum += tab[i * R + r];
        if (sum) atomicAdd((uint32_t*)(out + i), sum);   // inside the query's table: side * kMinkBins + i < 3 * kMinkBins
    }
#endif
}

void launch_sim_minkowski(hipStream_t st, const MinkowskiQueryDev* d_qs, int count, int max_groups, uint32_t* tables) {
    hipLaunchKernelGGL(k_minkowski, dim3((unsigned)max_groups, (unsigned)kMinkowskiSides, (unsigned)count), dim3(kStudyThreads), 0, st, d_qs, tables);
}

}  // namespace musica
