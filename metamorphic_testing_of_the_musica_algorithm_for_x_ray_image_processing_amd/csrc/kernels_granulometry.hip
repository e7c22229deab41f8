// kernels_granulometry.hip — the size metric of the study (musica_sim_granulometry, include/musica.h; metrics.granulometry_statistics):
// the granulometry (Matheron 1975; the pattern spectrum of Maragos 1989) of both sides of a comparison. For a radius r the element is
// the (2 r + 1)^2 square, clipped to the REGION: erosion = the minimum over it, dilation = the maximum, opening g_r = dilation of the
// erosion, closing = erosion of the dilation, g_0 = identity. For K ascending radii r_1 < .. < r_K <= 16 (r_0 = 0) class k < K of the
// bright polarity is A = g_{r_k}(a) - g_{r_k+1}(a), the residue class K is g_{r_K}(a); the dark polarity is the same of the closings,
// which are the openings of the complemented bytes (255 - closing_r(f) = g_r(255 - f)): ONE code for both, on complemented bytes for
// the dark one. Per class and polarity the five sums of A, B, A^2, B^2, A B over the region's pixels. Side a is the graded f32 plane of
// a batch image quantised with out_u8 while it is read (load_quant4: exactly what k_sim reads), side b a reference slot. No float
// arithmetic anywhere.
//
// k_granulometry: a query owns blockIdx.z, blockIdx.y is the polarity, and `groups` PERSISTENT workgroups of kStudyThreads threads share
// the 64 x 64 tiles of the region (tile_geom): workgroup g takes the tiles g, g + groups, ... Per tile:
//   stage     the (64 + 2 H)^2 window of BOTH sides, H = 2 r_K rounded up to a multiple of 4 (the tile starts on a word), as packed
//             bytes in LDS (stage_halo_window), 255 where the window leaves the region: the neutral value of a minimum, so that the
//             minimum over the window's square IS the minimum over the square clipped to the region. No pixel outside the region is read.
//   erode     the planes E are eroded in place from class to class: on a rectangle e_{r + s} = e_s e_r holds with the clipped element
//             too (the clamp of a pixel of the larger square towards the centre stays inside the rectangle), so class k erodes class
//             k - 1's planes by r_k - r_k-1.
//   dilate    the planes T = E with 0 outside the region (the neutral value of a maximum: E is not 0 there, it is the minimum of the
//             region's pixels nearby) are dilated by r_k: T is g_{r_k} on the tile.
//   sum       thread t keeps g_{r_k-1} of its 16 pixels (16 (t & 3) .. + 15 of tile row t / 4) of both sides in eight registers, so
//             A = previous - current is one u32 subtraction a word (opening decreases with r: no byte borrows), masked to the tile's
//             pixels inside the region; the five sums are v_dot4_u32_u8 (a tile's sum of A^2 is below 2^28), reduced over the
//             wavefront by DPP adds (wave_isum) and added to the workgroup's u64 table in LDS, which lives over all its tiles.
//   flush     once a workgroup: one u64 global atomic a word of the query's table, which the caller zeroes on the stream.
// WHAT IS VALID WHERE. The window's edge inside the region cuts squares off that the contract does not cut: a pass treats what lies
// beyond the window as absent. After the erosions up to r_k the planes E are exact where the window's edge is at least r_k away (or
// is the region's), the dilation by r_k needs E within r_k of the tile, H - r_k >= r_k from the edge. Nothing else is used.
// A PASS. A running extremum of length 2 s + 1 along one axis is O(log s) passes, not 2 s + 1 taps: F_1 = the plane,
// F_2j[x] = op(F_j[x], F_j[x + j]) up to the largest power of two p <= 2 s + 1, then out[x] = op(F_p[x - s], F_p[x + s - p + 1]):
// two overlapping windows of p that cover [x - s, x + s]. Every pass is "the op of two shifted reads", in place: all threads read,
// barrier, all write, barrier. A plane has 128 rows of 32 words (128 bytes): thread t owns word t & 31 of the rows t / 32 + 8 j,
// j < 16, so the lanes of a wavefront read consecutive words (no bank conflict) and a thread's column guards are loop-invariant; a
// horizontal shift of o bytes is two neighbouring words and v_alignbyte_b32. The extremum of four packed bytes is two
// v_pk_min_u16 / v_pk_max_u16 on the even and the odd bytes. Both sides go through a pass together: half the barriers.
// LDS: 4 planes of 16 KiB (E and T of either side) + the table: 65896 bytes, two workgroups a compute unit. No scratch.
// Integer sums commute: the tables are exact and byte-identical from call to call and for any number of workgroups
// (MUSICA_GRANULOMETRY_GROUPS, musica_study.hip).
// MUSICA_GRANULOMETRY_DIRECT_TAPS (a devtools/build_variant.sh build, for the A/B of DESIGN.md section 4; not shipped) replaces the
// doubling passes with one pass of 2 s + 1 taps: 2.76 times slower at r = 16 and 1.58 times at the radii 1, 2, 4, 8, 16, equal at r = 1.
#include "study_device.h"

namespace musica {

constexpr int kGranPitch = 32;                                                 // words between a plane's rows
constexpr int kGranRows = kSimTile + 4 * kGranulometryMaxRadius;               // 128: the window's side at r_K = 16
constexpr int kGranItems = kGranRows * kGranPitch / kStudyThreads;             // 16 words of a plane a thread
constexpr int kGranPlane = kGranRows * kGranPitch;
static_assert(kSimTile == 64 && kStudyThreads == 256, "a thread takes 16 pixels of a tile row: four lanes a row, 64 rows");
static_assert(kGranRows == 4 * kGranPitch && kStudyThreads % kGranPitch == 0 && kGranItems * kStudyThreads == kGranPlane, "a thread owns one word column of a plane");

typedef unsigned short GranU16x2 __attribute__((ext_vector_type(2)));

// The minimum (maximum) of every byte of x and y: the even and the odd bytes as two u16 pairs
template <bool MAX>
__device__ __forceinline__ uint32_t gran_op(uint32_t x, uint32_t y) {
    const GranU16x2 xe = __builtin_bit_cast(GranU16x2, x & 0x00FF00FFu), ye = __builtin_bit_cast(GranU16x2, y & 0x00FF00FFu);
    const GranU16x2 xo = __builtin_bit_cast(GranU16x2, (x >> 8) & 0x00FF00FFu), yo = __builtin_bit_cast(GranU16x2, (y >> 8) & 0x00FF00FFu);
    const GranU16x2 e = MAX ? __builtin_elementwise_max(xe, ye) : __builtin_elementwise_min(xe, ye);
    const GranU16x2 o = MAX ? __builtin_elementwise_max(xo, yo) : __builtin_elementwise_min(xo, yo);
    return __builtin_bit_cast(uint32_t, e) | (__builtin_bit_cast(uint32_t, o) << 8);
}

// Rows y_lo <= y < y_hi and words w_lo <= w < w_hi of a plane
struct GranBox {
    int y_lo, y_hi, w_lo, w_hi;
};

// One pass over both planes, in place: word (y, w) of `out` becomes op(the plane shifted by o1, the plane shifted by o2), a shift being
// bytes along the row (HORIZ) or rows; what a shifted read finds outside `in` is the op's neutral value. Ends behind a barrier.
template <bool MAX, bool HORIZ>
__device__ __forceinline__ void gran_pass(uint32_t* __restrict__ pa, uint32_t* __restrict__ pb, int o1, int o2, const GranBox& in, const GranBox& out) {
    constexpr uint32_t NEUTRAL = MAX ? 0u : 0xFFFFFFFFu;
    const int w = threadIdx.x & (kGranPitch - 1), y0 = threadIdx.x / kGranPitch;
    const bool mine = w >= out.w_lo && w < out.w_hi;
    // HORIZ: the words n and n + 1 that hold the four bytes o on from the word's first, and whether they lie inside `in`
    const int n1 = w + (o1 >> 2), n2 = w + (o2 >> 2);
    const uint32_t s1 = (uint32_t)o1 & 3u, s2 = (uint32_t)o2 & 3u;
    const bool lo1 = n1 >= in.w_lo && n1 < in.w_hi, hi1 = n1 + 1 >= in.w_lo && n1 + 1 < in.w_hi;
    const bool lo2 = n2 >= in.w_lo && n2 < in.w_hi, hi2 = n2 + 1 >= in.w_lo && n2 + 1 < in.w_hi;
    const bool col_in = w >= in.w_lo && w < in.w_hi;
    uint32_t ra[kGranItems], rb[kGranItems];
#pragma unroll
    for (int j = 0; j < kGranItems; j++) {
        const int y = y0 + j * (kStudyThreads / kGranPitch);
        if (!(mine && y >= out.y_lo && y < out.y_hi)) continue;
        if (HORIZ) {
            const bool row_in = y >= in.y_lo && y < in.y_hi;
            const uint32_t* const qa = pa + y * kGranPitch;
            const uint32_t* const qb = pb + y * kGranPitch;
            const uint32_t a1l = row_in && lo1 ? qa[n1] : NEUTRAL, a1h = row_in && hi1 ? qa[n1 + 1] : NEUTRAL;
            const uint32_t a2l = row_in && lo2 ? qa[n2] : NEUTRAL, a2h = row_in && hi2 ? qa[n2 + 1] : NEUTRAL;
            const uint32_t b1l = row_in && lo1 ? qb[n1] : NEUTRAL, b1h = row_in && hi1 ? qb[n1 + 1] : NEUTRAL;
            const uint32_t b2l = row_in && lo2 ? qb[n2] : NEUTRAL, b2h = row_in && hi2 ? qb[n2 + 1] : NEUTRAL;
            ra[j] = gran_op<MAX>(__builtin_amdgcn_alignbyte(a1h, a1l, s1), __builtin_amdgcn_alignbyte(a2h, a2l, s2));
            rb[j] = gran_op<MAX>(__builtin_amdgcn_alignbyte(b1h, b1l, s1), __builtin_amdgcn_alignbyte(b2h, b2l, s2));
        } else {
            const int y1 = y + o1, y2 = y + o2;
            const bool in1 = col_in && y1 >= in.y_lo && y1 < in.y_hi, in2 = col_in && y2 >= in.y_lo && y2 < in.y_hi;
            ra[j] = gran_op<MAX>(in1 ? pa[y1 * kGranPitch + w] : NEUTRAL, in2 ? pa[y2 * kGranPitch + w] : NEUTRAL);
            rb[j] = gran_op<MAX>(in1 ? pb[y1 * kGranPitch + w] : NEUTRAL, in2 ? pb[y2 * kGranPitch + w] : NEUTRAL);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kGranItems; j++) {
        const int y = y0 + j * (kStudyThreads / kGranPitch);
        if (!(mine && y >= out.y_lo && y < out.y_hi)) continue;
        pa[y * kGranPitch + w] = ra[j];
        pb[y * kGranPitch + w] = rb[j];
    }
    __syncthreads();
}

#ifdef MUSICA_GRANULOMETRY_DIRECT_TAPS
// The straightforward form (a devtools/build_variant.sh build, for the A/B of DESIGN.md section 4; not shipped): ONE pass whose word
// is the op of all 2 s + 1 shifted reads, tap by tap from LDS.
template <bool MAX, bool HORIZ>
__device__ __forceinline__ void gran_extremum(uint32_t* __restrict__ pa, uint32_t* __restrict__ pb, int s, const GranBox& in, const GranBox& out) {
    constexpr uint32_t NEUTRAL = MAX ? 0u : 0xFFFFFFFFu;
    const int w = threadIdx.x & (kGranPitch - 1), y0 = threadIdx.x / kGranPitch;
    const bool mine = w >= out.w_lo && w < out.w_hi;
    uint32_t ra[kGranItems], rb[kGranItems];
#pragma unroll
    for (int j = 0; j < kGranItems; j++) {
        const int y = y0 + j * (kStudyThreads / kGranPitch);
        if (!(mine && y >= out.y_lo && y < out.y_hi)) continue;
        uint32_t a = NEUTRAL, b = NEUTRAL;
        for (int o = -s; o <= s; o++) {
            if (HORIZ) {
                const int n = w + (o >> 2);
                const uint32_t sh = (uint32_t)o & 3u;
                const bool lo = n >= in.w_lo && n < in.w_hi, hi = n + 1 >= in.w_lo && n + 1 < in.w_hi;
                a = gran_op<MAX>(a, __builtin_amdgcn_alignbyte(hi ? pa[y * kGranPitch + n + 1] : NEUTRAL, lo ? pa[y * kGranPitch + n] : NEUTRAL, sh));
                b = gran_op<MAX>(b, __builtin_amdgcn_alignbyte(hi ? pb[y * kGranPitch + n + 1] : NEUTRAL, lo ? pb[y * kGranPitch + n] : NEUTRAL, sh));
            } else {
                const int yy = y + o;
                const bool there = yy >= in.y_lo && yy < in.y_hi;
                a = gran_op<MAX>(a, there ? pa[yy * kGranPitch + w] : NEUTRAL);
                b = gran_op<MAX>(b, there ? pb[yy * kGranPitch + w] : NEUTRAL);
            }
        }
        ra[j] = a, rb[j] = b;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kGranItems; j++) {
        const int y = y0 + j * (kStudyThreads / kGranPitch);
        if (!(mine && y >= out.y_lo && y < out.y_hi)) continue;
        pa[y * kGranPitch + w] = ra[j];
        pb[y * kGranPitch + w] = rb[j];
    }
    __syncthreads();
}
#else
// The running extremum of length 2 s + 1 (s >= 1) along one axis of both planes, in place: the doubling passes over `in`, then the
// two overlapping windows into `out` (inside `in`). What lies outside `in` counts as absent.
template <bool MAX, bool HORIZ>
__device__ __forceinline__ void gran_extremum(uint32_t* __restrict__ pa, uint32_t* __restrict__ pb, int s, const GranBox& in, const GranBox& out) {
    for (int p = 1;;) {
        const bool last = 2 * p > 2 * s + 1;   // p is the largest power of two <= 2 s + 1
        gran_pass<MAX, HORIZ>(pa, pb, last ? -s : 0, last ? s - p + 1 : p, in, last ? out : in);
        if (last) break;
        p *= 2;
    }
}
#endif

// The five sums of a class from 16 pixels of either side, four bytes a word
__device__ __forceinline__ void gran_sums(const uint32_t (&A)[4], const uint32_t (&B)[4], uint32_t (&s)[kGranulometryWords]) {
#pragma unroll
    for (int i = 0; i < kGranulometryWords; i++) s[i] = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        s[0] = dot4(A[j], 0x01010101u, s[0]);
        s[1] = dot4(B[j], 0x01010101u, s[1]);
        s[2] = dot4(A[j], A[j], s[2]);
        s[3] = dot4(B[j], B[j], s[3]);
        s[4] = dot4(A[j], B[j], s[4]);
    }
}

__global__ __launch_bounds__(kStudyThreads) void k_granulometry(const GranulometryQueryDev* __restrict__ qs, GranulometryRadii radii, unsigned long long* __restrict__ tables) {
    __shared__ __attribute__((aligned(16))) uint32_t ea[kGranPlane], eb[kGranPlane], ta[kGranPlane], tb[kGranPlane];
    __shared__ unsigned long long tab[(kGranulometryMaxRadii + 1) * kGranulometryWords];
    const GranulometryQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.groups) return;   // whole workgroup: the grid is sized for the query with the most groups
    const int t = threadIdx.x, K = radii.count, dark = (int)blockIdx.y;   // 1 <= K <= 8
    const int H = (2 * radii.r[K - 1] + 3) & ~3;                          // 4 .. 32, a multiple of 4
    const int side = kSimTile + 2 * H, words = side >> 2;                 // <= 128 rows of <= 32 words
    for (int i = t; i < (K + 1) * kGranulometryWords; i += kStudyThreads) tab[i] = 0ull;

    const int row = t >> 2, c0 = 16 * (t & 3);                            // the thread's 16 pixels of the tile
    const int mine = (H + row) * kGranPitch + ((H + c0) >> 2);            // their four words in a plane
    const int w = t & (kGranPitch - 1), y0 = t / kGranPitch;              // the thread's word column of a plane (gran_pass)
    const GranBox whole{0, side, 0, words};
    const uint32_t flip = dark ? 0xFFFFFFFFu : 0u;
    const auto bytes = [flip](uint32_t v) { return v ^ flip; };

    const int tiles = q.tiles_x * q.tiles_y;
    for (int tile = blockIdx.x; tile < tiles; tile += q.groups) {
        const TileGeom g = tile_geom(tile, q.tiles_x, q.w, q.h);
        __syncthreads();   // the last tile's planes are read; the first time: the table is cleared
        const int ox = g.x0 - H, oy = g.y0 - H;   // the window's first pixel in the region
        const int x_lo = max(ox, 0), x_hi = min(ox + side, q.w), y_lo = max(oy, 0), y_hi = min(oy + side, q.h);
        stage_halo_window((const GlobalF32*)q.a, q.a_pitch, ox, oy, x_lo, x_hi, y_lo, y_hi, ea, kGranPitch, words, side, bytes, 0xFFFFFFFFu);
        stage_halo_window((const GlobalU8*)q.b, q.b_pitch, ox, oy, x_lo, x_hi, y_lo, y_hi, eb, kGranPitch, words, side, bytes, 0xFFFFFFFFu);
        __syncthreads();
        // the bytes of the thread's words that are pixels of the tile inside the region, and of its word column that are inside the region
        uint32_t valid[4], inside = 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            valid[j] = 0u;
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (row < g.th && c0 + 4 * j + b < g.tw) valid[j] |= 0xFFu << (8 * b);
        }
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int x = ox + 4 * w + b;
            if (x >= 0 && x < q.w) inside |= 0xFFu << (8 * b);
        }
        uint32_t PA[4], PB[4];   // the opening by the radius before of the thread's pixels: the planes themselves at first
#pragma unroll
        for (int j = 0; j < 4; j++) PA[j] = ea[mine + j] & valid[j], PB[j] = eb[mine + j] & valid[j];

        for (int k = 0; k <= K; k++) {
            uint32_t A[4], B[4];
            if (k < K) {
                const int r = radii.r[k], s = r - (k ? radii.r[k - 1] : 0);   // s >= 1
                gran_extremum<false, true>(ea, eb, s, whole, whole);
                gran_extremum<false, false>(ea, eb, s, whole, whole);
                // T = E inside the region and 0 outside, on the rows that the dilation reads
                const GranBox reach{H - r, H + kSimTile + r, 0, words};
                const GranBox across{H - r, H + kSimTile + r, H >> 2, (H + kSimTile) >> 2};
                const GranBox tile_box{H, H + kSimTile, H >> 2, (H + kSimTile) >> 2};
                if (w < words) {
#pragma unroll
                    for (int j = 0; j < kGranItems; j++) {
                        const int y = y0 + j * (kStudyThreads / kGranPitch);
                        if (y < reach.y_lo || y >= reach.y_hi) continue;
                        const uint32_t keep = oy + y >= 0 && oy + y < q.h ? inside : 0u;
                        ta[y * kGranPitch + w] = ea[y * kGranPitch + w] & keep;
                        tb[y * kGranPitch + w] = eb[y * kGranPitch + w] & keep;
                    }
                }
                __syncthreads();
                gran_extremum<true, true>(ta, tb, r, reach, across);
                gran_extremum<true, false>(ta, tb, r, across, tile_box);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t ca = ta[mine + j] & valid[j], cb = tb[mine + j] & valid[j];
                    A[j] = PA[j] - ca, B[j] = PB[j] - cb;   // per byte previous >= current: no borrow
                    PA[j] = ca, PB[j] = cb;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) A[j] = PA[j], B[j] = PB[j];   // the residue
            }
            uint32_t s5[kGranulometryWords];
            gran_sums(A, B, s5);
            wave_isum(s5[0], s5[1], s5[2], s5[3], s5[4]);
            if (wave_last()) {
#pragma unroll
                for (int i = 0; i < kGranulometryWords; i++) atomicAdd(&tab[k * kGranulometryWords + i], (unsigned long long)s5[i]);
            }
        }
    }
    __syncthreads();
    // table [class][polarity][word]
    GlobalU64* const out = (GlobalU64*)tables + q.table;
    for (int i = t; i < (K + 1) * kGranulometryWords; i += kStudyThreads) {
        const int k = i / kGranulometryWords, word = i - k * kGranulometryWords;
        atomicAdd((unsigned long long*)(out + (k * 2 + dark) * kGranulometryWords + word), tab[i]);
    }
}

void launch_sim_granulometry(hipStream_t st, const GranulometryQueryDev* d_qs, int count, int max_groups, const GranulometryRadii& radii, unsigned long long* tables) {
    hipLaunchKernelGGL(k_granulometry, dim3((unsigned)max_groups, 2u, (unsigned)count), dim3(kStudyThreads), 0, st, d_qs, radii, tables);
}

}  // namespace musica
