// kernels_contours.hip — the contour metric of the study (musica_sim_contours, include/musica.h; metrics.contour_statistics): the exact
// squared Euclidean distance from every contour pixel of one side of a comparison to the nearest contour pixel of the other, counted
// per distance up to a radius R <= 32, in both directions. The contour E of a side is the thinned Sobel edge set: M = gx^2 + gy^2 on
// the region's interior and 0 elsewhere, E = M >= tau and M > before and M >= after along the axis of the larger gradient component.
// Side a is the graded f32 plane of a batch image quantised with out_u8 while it is read (load_quant4: exactly what k_sim reads), side
// b a reference slot. The region is its own domain. No float arithmetic anywhere, no division, separate launches: no workgroup ever
// waits for another, and every loop's trip count follows from the arguments.
//
// k_contour_mask: a query owns blockIdx.z, a workgroup of kStudyThreads threads one 64 x 64 tile of the region (tile_geom); it makes
// the tile's contour of side a, then of side b (the byte plane needs both), each like this:
//   stage    the 68 x 68 window from (x0 - 2, y0 - 2), clipped to the region, as packed bytes in LDS (stage_halo_window): 18 words a row,
//            the last one beyond the window and 0. No pixel outside the region is read.
//   strength M of the 66 x 66 pixels from (x0 - 1, y0 - 1), which non-maximum suppression of the tile reads: a thread takes four
//            neighbouring pixels of a row, forms the column sums t + 2 m + b and differences b - t of its six columns ONCE
//            (k_gradients' grad_columns, at this window's pitch) and the four gx, gy from them. Whether a pixel lies in the region's
//            interior comes from its coordinates, not from the zero padding: M = 0 outside. The word of a pixel is
//            M | horizontal << 31 (M <= 1 300 500 < 2^21), one 16-byte LDS store a thread (rows of 68 words: 16-byte aligned).
//   thin     a wavefront owns 16 tile rows, a lane a column: the pixel's word, the two neighbours along its axis (consecutive lanes
//            read consecutive words of a row: no bank conflict), the rule, and ONE ballot turns the tile row into a u64.
//   store    the 64 words of a side go to its bit plane in the scratch, h rows of ceil(w / 64) words (a tile column IS a word; bits
//            beyond w are 0 because the rule is false outside the tile's pixels), their popcounts, summed by DPP adds, to
//            counts[query][side] with one atomic a tile, and, where asked for, bit 0 | bit 1 << 1 to the byte plane.
// k_contour_distance: a query owns blockIdx.z, blockIdx.y is the direction (0: the sources are side a's contour, the targets side
// b's; 1: the other way round), and `groups` PERSISTENT workgroups share the region's tiles: workgroup g takes the tiles g,
// g + groups, ... Per tile:
//   stage    the target's bit rows y0 - R .. y0 + 63 + R and word columns tx - 1 .. tx + 1 as u64 in LDS, 0 outside the region: at most
//            128 x 3 words. The tile's 64 source words beside them.
//   compact  contours are sparse (a few percent of the pixels), so threads take list entries, they do not own a pixel: the first
//            wavefront turns the rows' popcounts into their exclusive prefix (one shuffle scan), then a lane per column gives a set
//            bit the ordinal prefix[row] + popcount(word & below the lane) and stores x | y << 6 there: a u16 list of at most 4096.
//   nearest  per entry the rows dy = 0, +1, -1, +2, .. are walked until dy^2 >= the best d^2 so far (no nearer pixel can follow) or
//            |dy| > R: at most 2 R + 1 rows. In a row the bits x .. x + R and x - R .. x are two u64 funnelled out of the three
//            staged words (R <= 32: a half with the centre fits one word), the nearest set bit a count of trailing / leading zeros,
//            the candidate dy^2 + dx^2. A source without a target within R gets the far bin R^2 + 1.
//   count    the bins go into a u32 table of R^2 + 2 words in LDS that lives over all the workgroup's tiles. THE 32-BIT RULE: a word
//            counts at most the pixels of one query, below 16384^2 = 2^28. Registered comparisons put most pixels into the bins 0, 1
//            and 2, so those are counted by one ballot and popcount each per wavefront and added by one lane, not by per-pixel
//            atomics on one address; every other bin takes an LDS atomic.
//   flush    once a workgroup: one u64 global atomic a TOUCHED word of the query's table, which the caller zeroes on the stream.
// Integer sums commute: the tables are exact and byte-identical from call to call and for any number of workgroups
// (MUSICA_CONTOURS_GROUPS, musica_study.hip).
// MUSICA_CONTOURS_PER_PIXEL (a devtools/build_variant.sh build, for the A/B of DESIGN.md section 4; not shipped) is the plain form of
// count and compact: a lane owns a pixel of the tile, no list, an LDS atomic for every bin.
#include "study_device.h"

namespace musica {

constexpr int kContourWinWords = 18;                 // words of a staged window row: 68 pixels and one word of zeros
constexpr int kContourWinRows = kSimTile + 4;        // 68
constexpr int kContourMSide = kSimTile + 2;          // 66: the pixels whose strength a tile's thinning reads
constexpr int kContourMPitch = 68;                   // words between rows of the strengths: 16-byte aligned rows
constexpr int kContourGroups4 = (kContourMSide + 3) / 4;   // 17 groups of four pixels a row
constexpr int kContourTgtRows = kSimTile + 2 * kContoursMaxRadius;   // 128
constexpr uint32_t kContourHorizontal = 0x80000000u;
static_assert(kSimTile == 64 && kStudyThreads == 256, "a tile row is one ballot word; a wavefront owns 16 rows");
static_assert(kContourGroups4 + 1 <= kContourWinWords && 4 * kContourGroups4 <= kContourMPitch && kContourMPitch % 4 == 0, "a group reads two words and stores four");
static_assert(kContoursMaxThreshold < kContourHorizontal, "the axis bit is free");
static_assert(kContoursMaxRadius <= 32, "the bits x .. x + R of a row fit one u64 with room to spare");

// The contour of one side on the tile g: rows[ty], ty < 64, become the ballot words (0 for ty >= g.th). win, m: the workgroup's LDS.
template <typename Px>
__device__ __forceinline__ void contour_tile(const Px* __restrict__ p, int pitch_px, const TileGeom& g, int w, int h, uint32_t tau, uint32_t* __restrict__ win,
                                             uint32_t* __restrict__ m, unsigned long long* __restrict__ rows) {
    const int t = threadIdx.x;
    const int ox = g.x0 - 2, oy = g.y0 - 2;
    stage_halo_window(p, pitch_px, ox, oy, max(ox, 0), min(ox + kContourWinRows, w), max(oy, 0), min(oy + kContourWinRows, h), win, kContourWinWords, kContourWinWords,
                      kContourWinRows, [](uint32_t v) { return v; });
    __syncthreads();
    for (int i = t; i < kContourMSide * kContourGroups4; i += kStudyThreads) {   // 1122 items: five trips
        const int r = i / kContourGroups4, grp = i - r * kContourGroups4;
        // strength row r, columns 4 grp .. + 3 = region pixels (x0 - 1 + 4 grp + k, y0 - 1 + r): window rows r .. r + 2, columns 4 grp .. + 5
        const uint32_t* q = win + r * kContourWinWords + grp;
        const uint32_t top[2] = {q[0], q[1]}, mid[2] = {q[kContourWinWords], q[kContourWinWords + 1]}, bot[2] = {q[2 * kContourWinWords], q[2 * kContourWinWords + 1]};
        int s[6], d[6];
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const int sh = 8 * (c & 3);
            const int tt = (int)((top[c >> 2] >> sh) & 0xFFu), mm = (int)((mid[c >> 2] >> sh) & 0xFFu), bb = (int)((bot[c >> 2] >> sh) & 0xFFu);
            s[c] = tt + 2 * mm + bb;
            d[c] = bb - tt;
        }
        const int y = g.y0 - 1 + r;
        const bool row_in = y >= 1 && y <= h - 2;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = g.x0 - 1 + 4 * grp + k;
            const int gx = s[k + 2] - s[k], gy = d[k] + 2 * d[k + 1] + d[k + 2];
            const uint32_t strength = (uint32_t)(gx * gx + gy * gy);
            v[k] = row_in && x >= 1 && x <= w - 2 ? strength | (abs(gx) >= abs(gy) ? kContourHorizontal : 0u) : 0u;
        }
        *reinterpret_cast<uint4*>(m + r * kContourMPitch + 4 * grp) = make_uint4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
    const int lane = t & 63, wave = t >> 6;
    for (int k = 0; k < kSimTile / kStudyWaves; k++) {
        const int ty = wave * (kSimTile / kStudyWaves) + k;
        const uint32_t* c = m + (ty + 1) * kContourMPitch + lane + 1;   // the pixel's own word
        const uint32_t own = c[0], strength = own & ~kContourHorizontal;
        const bool horizontal = (own & kContourHorizontal) != 0u;
        const uint32_t before = (horizontal ? c[-1] : c[-kContourMPitch]) & ~kContourHorizontal;
        const uint32_t after = (horizontal ? c[1] : c[kContourMPitch]) & ~kContourHorizontal;
        const bool edge = ty < g.th && lane < g.tw && strength >= tau && strength > before && strength >= after;
        const unsigned long long word = __ballot(edge);
        if (lane == 0) rows[ty] = word;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kStudyThreads) void k_contour_mask(const ContourQueryDev* __restrict__ qs, uint32_t tau, unsigned long long* __restrict__ bits,
                                                                 unsigned long long* __restrict__ counts, uint8_t* __restrict__ planes) {
    __shared__ __attribute__((aligned(16))) uint32_t win[kContourWinRows * kContourWinWords];
    __shared__ __attribute__((aligned(16))) uint32_t m[kContourMSide * kContourMPitch];
    __shared__ unsigned long long rows[2][kSimTile];
    const ContourQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.tiles_x * q.tiles_y) return;   // whole workgroup: the grid is sized for the query with the most tiles
    const TileGeom g = tile_geom(blockIdx.x, q.tiles_x, q.w, q.h);
    const int t = threadIdx.x, tx = g.x0 / kSimTile;
    contour_tile((const GlobalF32*)q.a, q.a_pitch, g, q.w, q.h, tau, win, m, rows[0]);
    contour_tile((const GlobalU8*)q.b, q.b_pitch, g, q.w, q.h, tau, win, m, rows[1]);
    if (t < 2 * kSimTile) {   // the first two wavefronts, whole: side t >> 6, tile row t & 63
        const int side = t >> 6, ty = t & 63;
        const unsigned long long word = rows[side][ty];   // 0 for ty >= g.th
        if (ty < g.th) ((GlobalU64*)bits)[q.bits + ((size_t)side * q.h + g.y0 + ty) * q.row_words + tx] = word;
        uint32_t n = (uint32_t)__popcll(word);
        wave_isum(n);
        if (wave_last() && n) atomicAdd(counts + 2 * blockIdx.z + side, (unsigned long long)n);
    }
    if (planes) {
        GlobalU8* const out = (GlobalU8*)planes + q.plane;
        for (int i = t; i < kSimTile * kSimTile; i += kStudyThreads) {
            const int ty = i >> 6, x = i & 63;
            if (ty < g.th && x < g.tw)
                out[(size_t)(g.y0 + ty) * q.w + g.x0 + x] = (uint8_t)(((rows[0][ty] >> x) & 1ull) | (((rows[1][ty] >> x) & 1ull) << 1));
        }
    }
}

// The squared distance from tile pixel (x, y) to the nearest target bit within R, or R^2 + 1: tgt[row][3] holds the target's bit rows
// from y0 - R on and its word columns tx - 1 .. tx + 1, so the pixel is bit 64 + x of row y + R.
__device__ __forceinline__ uint32_t contour_nearest(const unsigned long long* __restrict__ tgt, int x, int y, int R) {
    const uint32_t far = (uint32_t)(R * R + 1);
    const unsigned long long right_mask = (2ull << R) - 1ull, left_mask = ~0ull << (63 - R);   // R + 1 bits from the centre on, either way
    uint32_t best = far;
    for (int a = 0; a <= R; a++) {   // |dy|
        const uint32_t aa = (uint32_t)(a * a);
        if (aa >= best) break;       // every row from here on is at least this far
        for (int sgn = 0; sgn < (a ? 2 : 1); sgn++) {
            const unsigned long long* row = tgt + (y + R + (sgn ? -a : a)) * 3;
            const unsigned long long w0 = row[0], w1 = row[1], w2 = row[2];
            // bit k of `right` is the pixel x + k, bit 63 - k of `left` the pixel x - k
            const unsigned long long right = ((w1 >> x) | (x ? w2 << (64 - x) : 0ull)) & right_mask;
            const unsigned long long left = (x == 63 ? w1 : (w0 >> (x + 1)) | (w1 << (63 - x))) & left_mask;
            uint32_t dx = 64u;
            if (right) dx = (uint32_t)__builtin_ctzll(right);
            if (left) dx = min(dx, (uint32_t)__builtin_clzll(left));
            if (dx <= (uint32_t)R) best = min(best, aa + dx * dx);
        }
    }
    return best < far ? best : far;   // a candidate beyond the radius (dy^2 + dx^2 > R^2) is far as well
}

__global__ __launch_bounds__(kStudyThreads) void k_contour_distance(const ContourQueryDev* __restrict__ qs, int R, const unsigned long long* __restrict__ bits,
                                                                     unsigned long long* __restrict__ tables) {
    __shared__ unsigned long long tgt[kContourTgtRows * 3];
    __shared__ unsigned long long src[kSimTile];
    __shared__ uint32_t tab[kContoursMaxRadius * kContoursMaxRadius + 2];
#ifndef MUSICA_CONTOURS_PER_PIXEL
    __shared__ uint32_t prefix[kSimTile + 1];
    __shared__ uint16_t list[kSimTile * kSimTile];
#endif
    const ContourQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.groups) return;   // whole workgroup: the grid is sized for the query with the most groups
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, dir = (int)blockIdx.y, bins = R * R + 2;
    const GlobalU64* const sbits = (const GlobalU64*)bits + q.bits + (size_t)dir * q.h * q.row_words;
    const GlobalU64* const tbits = (const GlobalU64*)bits + q.bits + (size_t)(1 - dir) * q.h * q.row_words;
    for (int i = t; i < bins; i += kStudyThreads) tab[i] = 0u;
    uint32_t low[3] = {0u, 0u, 0u};   // a wavefront's first lane: its pixels of the bins 0, 1, 2
    const int tiles = q.tiles_x * q.tiles_y, rows = kSimTile + 2 * R;
    for (int tile = blockIdx.x; tile < tiles; tile += q.groups) {
        const int ty0 = tile / q.tiles_x, tx = tile - ty0 * q.tiles_x, y0 = ty0 * kSimTile;
        __syncthreads();   // the last tile's words are read; the first time: the table is cleared
        for (int i = t; i < rows * 3; i += kStudyThreads) {
            const int r = i / 3, k = i - r * 3;
            const int y = y0 - R + r, wx = tx - 1 + k;
            tgt[i] = y >= 0 && y < q.h && wx >= 0 && wx < q.row_words ? tbits[(size_t)y * q.row_words + wx] : 0ull;
        }
        if (t < kSimTile) src[t] = y0 + t < q.h ? sbits[(size_t)(y0 + t) * q.row_words + tx] : 0ull;
        __syncthreads();
#ifdef MUSICA_CONTOURS_PER_PIXEL
        for (int k = 0; k < kSimTile / kStudyWaves; k++) {
            const int y = wave * (kSimTile / kStudyWaves) + k;
            if ((src[y] >> lane) & 1ull) atomicAdd(&tab[contour_nearest(tgt, lane, y, R)], 1u);
        }
#else
        if (wave == 0) {   // the rows' popcounts to their exclusive prefix; prefix[64]: the tile's contour pixels
            const uint32_t n = (uint32_t)__popcll(src[lane]);
            uint32_t inc = n;
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t o = __shfl_up(inc, off, 64);
                if (lane >= off) inc += o;
            }
            prefix[lane] = inc - n;
            if (lane == 63) prefix[kSimTile] = inc;
        }
        __syncthreads();
        for (int k = 0; k < kSimTile / kStudyWaves; k++) {
            const int y = wave * (kSimTile / kStudyWaves) + k;
            const unsigned long long word = src[y];
            if ((word >> lane) & 1ull) list[prefix[y] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull))] = (uint16_t)(lane | (y << 6));
        }
        __syncthreads();
        const int n = (int)prefix[kSimTile];   // <= 4096
        for (int base = 0; base < n; base += kStudyThreads) {   // uniform over the workgroup: the ballots below see whole wavefronts
            const int i = base + t;
            uint32_t bin = 0xFFFFFFFFu;
            if (i < n) {
                const int e = list[i];
                bin = contour_nearest(tgt, e & 63, e >> 6, R);
            }
#pragma unroll
            for (int b = 0; b < 3; b++) low[b] += (uint32_t)__popcll(__ballot(bin == (uint32_t)b));   // every lane counts; the first one's is used
            if (bin >= 3u && bin != 0xFFFFFFFFu) atomicAdd(&tab[bin], 1u);
        }
#endif
    }
#ifndef MUSICA_CONTOURS_PER_PIXEL
    if (lane == 0) {   // bins <= 2 means R = 1 with the bins 0, 1 and far = 2: all three exist for every R >= 1
#pragma unroll
        for (int b = 0; b < 3; b++)
            if (low[b]) atomicAdd(&tab[b], low[b]);
    }
#endif
    __syncthreads();
    GlobalU64* const out = (GlobalU64*)tables + q.table + (size_t)dir * bins;
    for (int i = t; i < bins; i += kStudyThreads)
        if (tab[i]) atomicAdd((unsigned long long*)(out + i), (unsigned long long)tab[i]);
}

void launch_sim_contours(hipStream_t st, const ContourQueryDev* d_qs, int count, int max_tiles, int max_groups, uint32_t threshold, int radius,
                         unsigned long long* bits, unsigned long long* counts, uint8_t* planes, unsigned long long* tables) {
    hipLaunchKernelGGL(k_contour_mask, dim3((unsigned)max_tiles, 1u, (unsigned)count), dim3(kStudyThreads), 0, st, d_qs, threshold, bits, counts, planes);
    hipLaunchKernelGGL(k_contour_distance, dim3((unsigned)max_groups, 2u, (unsigned)count), dim3(kStudyThreads), 0, st, d_qs, radius, bits, tables);
}

}  // namespace musica
