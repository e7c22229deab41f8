// kernels_reach.hip — the reach metric of the study (musica_sim_reach / musica_sim_reach_classes, include/musica.h; metrics.reach_classes,
// metrics.reach_statistics): the exact sums of a comparison kept apart by the Chebyshev distance of the pixel from the nearest CHANGED
// pixel of the input, seed = source != altered. A pixel is within r of a seed exactly when the (2r + 1)^2 box around it, clipped to the
// plane, holds one, and one summed-area table of the seed mask answers that with four loads: no distance transform, no propagation, no
// atomics before the sums, no float. Exact for every size and every mask.
//
// THE TABLE. S[y][x] = the seeds of rows 0 .. y, columns 0 .. x, n x n u32 (n^2 <= 2^28 seeds fit), INDEX GUARDS in place of an
// (n + 1)^2 table: a box [xa, xb] x [ya, yb], xb and yb clipped to n - 1, holds S[yb][xb] - S[yb][xa - 1] - S[ya - 1][xb] +
// S[ya - 1][xa - 1] seeds, a term with an index of -1 being 0 (reach_count: the four loads are unconditional, on clamped addresses
// inside the plane, and the terms are masked). S[n - 1][n - 1] is the number of seeds.
//   k_reach_rows<V>  a workgroup of kStudyThreads threads owns ONE row. A thread takes chunks of V consecutive pixels of both planes
//                    (study_device.h's pixel words: V = 8, one 16-byte load a plane, where n % 8 == 0 and both planes are 16-byte
//                    aligned, else 2, else 1), counts its chunk's seeds, the workgroup scans the threads' counts (block_scan_exclusive)
//                    and the thread stores its V inclusive counts as one 32-, 8- or 4-byte store. A row longer than kStudyThreads V
//                    pixels takes further trips with the count so far carried. 4 bytes read, 4 written per pixel.
//   k_reach_cols     the running sums down the columns, IN PLACE. A workgroup owns 64 columns, a lane one column, so every access is a
//                    coalesced row segment; its kReachColWaves wavefronts cut the rows into as many segments. Pass 1 sums each segment
//                    (independent loads), the segments' totals meet in LDS, pass 2 walks each segment again from the total of those
//                    above it (the segment, 64 columns x n / 16 rows x 4 bytes, is still in the L2) and stores. 8 bytes read, 4 written.
//
// THE CLASS of pixel (x, y) is the smallest k with a seed inside the box of radii[k], K where the box of radii[K - 1] holds none
// (radii ascending from radii[0] = 0: class 0 is a seed itself). "The box holds a seed" is monotone in the radius, so the class is found
// by bisection over the K radii (reach_bisect): at most 6 steps of four S loads for 32 radii, the radii read from LDS.
//   THE TILE BOUNDS. A workgroup owns a 64 x 64 tile [x0, x1] x [y0, y1]. From below: the tile grown by radii[k] contains the box of
//   radii[k] of every pixel of the tile, so where the grown tile holds no seed, no pixel of the tile has a class <= k; `lo` is the
//   smallest k whose grown tile holds a seed (K if none does). From above: the box of radius r of every pixel of the tile contains
//   [x1 - r, x0 + r] x [y1 - r, y0 + r] (not empty from 2r >= the tile's larger side - 1 on), so where that core holds a seed every
//   pixel has a class <= k; `hi` is the smallest such k (K if none). Both are found first, by the same bisection on uniform values
//   (both predicates are monotone in r), and every pixel's bisection runs over lo .. hi only. The bounds narrow the search and nothing
//   else: a class never depends on them. A tile far from every seed, where d - 63 and d + 63 fall into one or two classes, takes one
//   step or none, which is where the large boxes with their four far-apart loads would be.
//
// k_sim_reach: metrics.reach_statistics. A query owns blockIdx.z, a workgroup one 64 x 64 tile of its region (tile_geom). Side a is the
// graded f32 plane of a batch image quantised with out_u8 while it is read (load_quant4: exactly what k_sim reads), side b a reference
// slot, the class that of the input pixel under side a's pixel. A thread takes four neighbouring pixels of a row, sixteen lanes a tile
// row, four rows a wavefront, four trips a tile.
//   THE ACCUMULATION, as k_gradients': no per-pixel atomics. Per trip a wavefront walks the classes between the tile bounds and skips,
//   with one ballot each, those that none of its 256 pixels has; for a class that is present every lane sums its pixels of that class,
//   n, changed, sum a, sum b and sum (a - b)^2 go through ONE wave_isum and max |a - b| through wave_umax (DPP, no LDS traffic), and
//   the wavefront's last lane adds them, with plain LDS adds and a maximum, into the wavefront's OWN [K + 1][6] table of 32-bit words.
//   THE 32-BIT RULE. A wavefront counts at most kReachWavePixels = 16 rows x 64 columns = 1024 pixels of a tile, so a word of its table
//   is at most 1024 x 255^2 = 66 585 600 < 2^32 (asserted below). The four tables are widened to 64 bits where they are combined, one
//   table word a thread, and the non-zero words go to the query's table with 64-bit integer global atomics, atomicAdd for the five sums
//   and atomicMax for max |a - b| (the caller zeroes the tables on the stream). Integer sums and maxima commute: exact and identical
//   from call to call in any order.
//   A workgroup a tile, on purpose: every workgroup ends with up to (K + 1) x 6 atomics on the same words of its query's table, but
//   a form in which at most 256 workgroups a query strode over the tiles, a ninth of the atomics at 3072^2, was SLOWER (MEASURED,
//   318 us against 203): the launch lives on the latency of the dependent table loads that many resident
//   workgroups hide, not on the atomics.
// k_reach_classes: the class plane itself, cropped by the margin: a workgroup per 64 x 64 tile of the cropped plane, a thread one pixel
// of a row at a time (coalesced byte stores), the same tile bounds and bisection.
// Nothing outside the planes named is read or written.
#include "study_device.h"

namespace musica {

constexpr int kReachColWaves = 16;                                    // row segments of a column workgroup
constexpr int kReachLanes = kSimTile / 4;                             // lanes of a tile row, four pixels each
constexpr int kReachRows = kStudyThreads / kReachLanes;               // tile rows of a trip
constexpr int kReachTrips = kSimTile / kReachRows;
constexpr int kReachWavePixels = kSimTile * kSimTile / kStudyWaves;   // what a wavefront counts of a tile
constexpr int kReachMaxClasses = kReachMaxRadii + 1;
static_assert(kReachLanes == 16 && kReachRows == 16 && kReachTrips == 4, "16 lanes a row, 4 rows a wavefront, 4 trips a tile");
static_assert(kReachWavePixels == 1024 && kReachWavePixels * 255ull * 255ull < (1ull << 32), "THE 32-BIT RULE: a wavefront's share of a tile fits a 32-bit word");
static_assert(kReachMaxClasses * kReachWords <= kStudyThreads, "one table word a thread");
static_assert(16384ull * 16384ull < (1ull << 32) && kReachMaxRadius + 16384 < (1 << 30), "S is u32 and a box's corners are ints for every plane a context accepts");

// ---- the table ---------------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(kStudyThreads) void k_reach_rows(const uint16_t* __restrict__ src, const uint16_t* __restrict__ alt, uint32_t* __restrict__ sat, int n) {
    typedef typename PixelWord<V>::type __attribute__((may_alias)) Word;
    __shared__ uint32_t wave_tot[kStudyWaves];
    const size_t row = (size_t)blockIdx.x * n;
    uint32_t carry = 0u;
    for (int c0 = 0; c0 < n; c0 += kStudyThreads * V) {   // uniform: every thread reaches the scan's barriers
        const int x = c0 + (int)threadIdx.x * V;           // n % V == 0: a chunk starts inside the row or lies outside it entirely
        uint32_t inc[V], run = 0u;
        if (x < n) {
            PixelChunk<V> a, b;
            a.w = *reinterpret_cast<const Word*>(src + row + x);
            b.w = *reinterpret_cast<const Word*>(alt + row + x);
#pragma unroll
            for (int i = 0; i < V; i++) {
                run += a.px[i] != b.px[i] ? 1u : 0u;
                inc[i] = run;
            }
        }
        uint32_t total;
        const uint32_t before = carry + block_scan_exclusive(run, wave_tot, &total);
        carry += total;
        if (x < n) {
            uint32_t* o = sat + row + x;   // (row + x) % V == 0: the store is naturally aligned
            if constexpr (V == 8) {
                reinterpret_cast<uint4*>(o)[0] = make_uint4(before + inc[0], before + inc[1], before + inc[2], before + inc[3]);
                reinterpret_cast<uint4*>(o)[1] = make_uint4(before + inc[4], before + inc[5], before + inc[6], before + inc[7]);
            } else if constexpr (V == 2) {
                *reinterpret_cast<uint2*>(o) = make_uint2(before + inc[0], before + inc[1]);
            } else {
                *o = before + inc[0];
            }
        }
    }
}

// blockDim = (64, kReachColWaves): threadIdx.x the column of the workgroup's 64, threadIdx.y the row segment
__global__ __launch_bounds__(64 * kReachColWaves) void k_reach_cols(uint32_t* sat, int n) {
    __shared__ uint32_t seg_tot[kReachColWaves][64];
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, w = (int)threadIdx.y;
    const int seg = (n + kReachColWaves - 1) / kReachColWaves;
    const int y0 = min(w * seg, n), y1 = min(y0 + seg, n);
    uint32_t* col = sat + min(x, n - 1);   // a column outside the plane reads the last one and stores nothing
    uint32_t sum = 0u;
#pragma unroll 8
    for (int y = y0; y < y1; y++) sum += col[(size_t)y * n];
    seg_tot[w][threadIdx.x] = sum;
    __syncthreads();
    if (x >= n) return;
    uint32_t run = 0u;
    for (int k = 0; k < w; k++) run += seg_tot[k][threadIdx.x];
#pragma unroll 8
    for (int y = y0; y < y1; y++) {
        run += col[(size_t)y * n];
        col[(size_t)y * n] = run;
    }
}

void launch_reach_table(hipStream_t st, const uint16_t* source, const uint16_t* altered, uint32_t* sat, int n) {
    launch_by_width(
        [&](auto v) {
            constexpr int V = decltype(v)::value;
            hipLaunchKernelGGL((k_reach_rows<V>), dim3((unsigned)n), dim3(kStudyThreads), 0, st, source, altered, sat, n);
        },
        n, source, altered);
    hipLaunchKernelGGL(k_reach_cols, dim3((unsigned)((n + 63) / 64)), dim3(64, kReachColWaves), 0, st, sat, n);
}

// ---- the class ---------------------------------------------------------------------------------------------------------------------------
// The seeds inside [xa, xb] x [ya, yb] clipped to the n x n plane; xa <= xb, ya <= yb, xa, ya <= n - 1 and xb, yb >= 0 (a box around a
// pixel of the plane, or what lies between two of them). Modulo 2^32 on the way, exact at the end.
__device__ __forceinline__ uint32_t reach_count(const GlobalU32* __restrict__ S, int n, int xa, int ya, int xb, int yb) {
    xb = min(xb, n - 1);
    yb = min(yb, n - 1);
    const bool left = xa > 0, top = ya > 0;
    const int xl = max(xa, 1) - 1, yt = max(ya, 1) - 1;   // inside the plane also where the term is masked
    const uint32_t d = S[(size_t)yb * n + xb], c = S[(size_t)yb * n + xl], b = S[(size_t)yt * n + xb], a = S[(size_t)yt * n + xl];
    return d - (left ? c : 0u) - (top ? b : 0u) + (left && top ? a : 0u);
}

// The smallest k in lo .. hi - 1 for which the rectangle [xa, xb] x [ya, yb] grown by radii[k] holds a seed, hi where none does. The
// rectangle may be given inside out (xa > xb or ya > yb: the core of THE TILE BOUNDS): it holds nothing until it has grown right.
__device__ __forceinline__ int reach_bisect(const GlobalU32* __restrict__ S, int n, int xa, int ya, int xb, int yb, const uint32_t* __restrict__ radii, int lo, int hi) {
    int l = lo, h = hi;
    while (l < h) {
        const int m = (l + h) >> 1, r = (int)radii[m];
        if (xa - r <= xb + r && ya - r <= yb + r && reach_count(S, n, xa - r, ya - r, xb + r, yb + r) > 0u) h = m;
        else l = m + 1;
    }
    return l;
}

// THE TILE BOUNDS of the tile [x0, x0 + tw) x [y0, y0 + th) of the input plane (uniform over the workgroup)
struct ReachBounds {
    int lo, hi;
};
__device__ __forceinline__ ReachBounds reach_tile_bounds(const GlobalU32* __restrict__ S, int n, int x0, int y0, int tw, int th, const uint32_t* __restrict__ rad, int K) {
    const int x1 = x0 + tw - 1, y1 = y0 + th - 1;
    const int lo = reach_bisect(S, n, x0, y0, x1, y1, rad, 0, K);
    return {lo, reach_bisect(S, n, x1, y1, x0, y0, rad, lo, K)};   // the core inside out; it holds nothing the grown tile does not: hi >= lo
}

__global__ __launch_bounds__(kStudyThreads) void k_sim_reach(const ReachQueryDev* __restrict__ qs, const uint32_t* __restrict__ sat, int n, const uint32_t* __restrict__ d_radii,
                                                             int K, unsigned long long* __restrict__ tables) {
    __shared__ uint32_t rad[kReachMaxRadii];
    __shared__ uint32_t tab[kStudyWaves][kReachMaxClasses][kReachWords];
    const ReachQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.tiles_x * q.tiles_y) return;   // whole workgroup: the grid is sized for the query with the most tiles
    const GlobalU32* __restrict__ S = (const GlobalU32*)sat;
    const int t = threadIdx.x;
    for (int i = t; i < kStudyWaves * kReachMaxClasses * kReachWords; i += kStudyThreads) (&tab[0][0][0])[i] = 0u;
    if (t < K) rad[t] = d_radii[t];
    __syncthreads();
    const int cx = (t & (kReachLanes - 1)) * 4, r = t / kReachLanes;
    uint32_t* __restrict__ mine = &tab[t >> 6][0][0];
    const TileGeom g = tile_geom(blockIdx.x, q.tiles_x, q.w, q.h);
    const int px0 = q.sx + g.x0, py0 = q.sy + g.y0;   // the tile in the input plane
    const ReachBounds bound = reach_tile_bounds(S, n, px0, py0, g.tw, g.th, rad, K);
    const GlobalF32* __restrict__ pa = (const GlobalF32*)q.a + (ptrdiff_t)g.y0 * q.a_pitch + g.x0;
    const GlobalU8* __restrict__ pb = (const GlobalU8*)q.b + (ptrdiff_t)g.y0 * q.b_pitch + g.x0;
    for (int k = 0; k < kReachTrips; k++) {
        const int ty = k * kReachRows + r;
        const int npx = ty < g.th ? max(0, min(4, g.tw - cx)) : 0;
        uint32_t wa = 0u, wb = 0u;
        int cls[4] = {-1, -1, -1, -1};
        unsigned long long present = 0ull;
        if (npx > 0) {
            wa = load_quant4(pa + (ptrdiff_t)ty * q.a_pitch + cx, npx);
            wb = load_bytes4(pb + (ptrdiff_t)ty * q.b_pitch + cx, npx);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (i >= npx) break;
                const int x = px0 + cx + i, y = py0 + ty;
                cls[i] = reach_bisect(S, n, x, y, x, y, rad, bound.lo, bound.hi);
                present |= 1ull << cls[i];
            }
        }
        for (int c = bound.lo; c <= bound.hi; c++) {
            if (__ballot((present >> c) & 1ull) == 0ull) continue;   // uniform over the wavefront
            uint32_t cn = 0u, ch = 0u, sa = 0u, sb = 0u, dd = 0u, mx = 0u;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (cls[i] != c) continue;
                const uint32_t a = (wa >> (8 * i)) & 0xFFu, b = (wb >> (8 * i)) & 0xFFu;
                const uint32_t d = a > b ? a - b : b - a;
                cn += 1u;
                ch += d ? 1u : 0u;
                sa += a;
                sb += b;
                dd += d * d;
                mx = d > mx ? d : mx;
            }
            wave_isum(cn, ch, sa, sb, dd);   // at most 256 pixels: every word below 2^25; all 64 lanes are here (the ballot is uniform)
            wave_umax(mx);
            if (wave_last()) {
                uint32_t* row = mine + c * kReachWords;
                row[0] += cn;
                row[1] += ch;
                row[2] += sa;
                row[3] += sb;
                row[4] += dd;
                row[5] = mx > row[5] ? mx : row[5];
            }
        }
    }
    __syncthreads();
    if (t < (K + 1) * kReachWords) {   // word f of class c, the four wavefronts widened to 64 bits
        const int c = t / kReachWords, f = t - c * kReachWords;
        unsigned long long v = 0ull;
        for (int w = 0; w < kStudyWaves; w++) {
            const unsigned long long o = tab[w][c][f];
            v = f == kReachWords - 1 ? (o > v ? o : v) : v + o;
        }
        unsigned long long* out = (unsigned long long*)((GlobalU64*)tables + q.table + (size_t)c * kReachWords + f);
        if (v) {
            if (f == kReachWords - 1) atomicMax(out, v);
            else atomicAdd(out, v);
        }
    }
}

__global__ __launch_bounds__(kStudyThreads) void k_reach_classes(const uint32_t* __restrict__ sat, int n, int margin, const uint32_t* __restrict__ d_radii, int K,
                                                                 uint8_t* __restrict__ dst) {
    __shared__ uint32_t rad[kReachMaxRadii];
    const int side = n - 2 * margin, tiles = (side + kSimTile - 1) / kSimTile;
    const TileGeom g = tile_geom(blockIdx.x, tiles, side, side);
    const GlobalU32* __restrict__ S = (const GlobalU32*)sat;
    const int px0 = margin + g.x0, py0 = margin + g.y0;
    if ((int)threadIdx.x < K) rad[threadIdx.x] = d_radii[threadIdx.x];
    __syncthreads();
    const ReachBounds bound = reach_tile_bounds(S, n, px0, py0, g.tw, g.th, rad, K);
    for (int e = threadIdx.x; e < kSimTile * kSimTile; e += kStudyThreads) {
        const int ty = e / kSimTile, tx = e - ty * kSimTile;
        if (ty >= g.th || tx >= g.tw) continue;
        const int x = px0 + tx, y = py0 + ty;
        dst[(size_t)(g.y0 + ty) * side + g.x0 + tx] = (uint8_t)reach_bisect(S, n, x, y, x, y, rad, bound.lo, bound.hi);
    }
}

void launch_sim_reach(hipStream_t st, const ReachQueryDev* d_qs, int count, int max_tiles, const uint32_t* sat, int n, const uint32_t* d_radii, int K,
                      unsigned long long* tables) {
    hipLaunchKernelGGL(k_sim_reach, dim3((unsigned)max_tiles, 1, (unsigned)count), dim3(kStudyThreads), 0, st, d_qs, sat, n, d_radii, K, tables);
}

void launch_reach_classes(hipStream_t st, const uint32_t* sat, int n, int margin, const uint32_t* d_radii, int K, uint8_t* dst) {
    const unsigned tiles = (unsigned)((n - 2 * margin + kSimTile - 1) / kSimTile);
    hipLaunchKernelGGL(k_reach_classes, dim3(tiles * tiles), dim3(kStudyThreads), 0, st, sat, n, margin, d_radii, K, dst);
}

}  // namespace musica
