// kernels_order.hip — the local-order metric of the study (musica_sim_order, include/musica.h; metrics.order_statistics): the census
// signs of both sides of a comparison over the interior of its region. For a pixel c and each of its 48 neighbours n within the 7 x 7
// neighbourhood, per side the sign of p[n] - p[c]; a (pixel, neighbour) pair is `same`, `reversed`, `flattened` (a ties, b orders),
// `split` (a orders, b ties) or tied on both sides, counted per ring max(|dx|, |dy|) = 1, 2, 3; and the histogram of the per-pixel
// census distance d = sum |sa - sb| = 2 reversed + flattened + split, 0 .. 96. Side a is the graded f32 plane of a batch image quantised
// with out_u8 while it is read (load_quant4: exactly what k_sim and k_gradients read), side b a reference slot. No float anywhere.
//
// k_order: a query owns blockIdx.z, a workgroup of kStudyThreads threads one 64 x 64 tile of the query's INTERIOR, the (w - 6) x
// (h - 6) pixels whose 7 x 7 neighbourhood lies inside the region (tile_geom over the interior).
//   stage    the (tw + 6) x (th + 6) windows of both sides, at most 70 x 70, once, as packed bytes in LDS (stage_windows): 18 words a
//            row, zeros beyond a ragged tile, nothing outside the region is read.
//   signs    a thread takes four neighbouring pixels of a row, sixteen lanes a tile row, four rows a wavefront, four trips a tile. It
//            reads three words of each of the seven window rows per side (ten bytes: the columns of its four neighbourhoods). Per pixel
//            and side it builds two masks of 48 bits, lt (n < c) and gt (n > c), one bit a neighbour: the bit is the sign bit of n - c
//            or c - n, shifted in with v_alignbit_b32. A mask is three words, one a ring (8, 16 and 24 bits from bit 0, the bits above
//            them 0: the neighbours are walked ring by ring, the loops are unrolled, so the order costs nothing).
//   counts   same = (lt_a & lt_b) | (gt_a & gt_b), reversed = (lt_a & gt_b) | (gt_a & lt_b), flattened = ~(lt_a | gt_a) & (lt_b | gt_b),
//            split = (lt_a | gt_a) & ~(lt_b | gt_b): one v_bcnt_u32_b32 a ring and category. A row or a pixel outside a ragged tile is
//            skipped by a branch: it counts nothing and costs nothing.
// THE ACCUMULATION. The ring sums need no per-pixel identity: a thread adds the twelve counts of its sixteen pixels in registers, at
// most 16 x 24 = 384 each, two counts a word (same | reversed << 16, flattened | split << 16: six words), the wavefront reduces them
// with ONE wave_isum a tile, six words interleaved, and its last lane stores the twelve counts into the wavefront's OWN row of 32-bit
// words in LDS. Only d is per pixel: one LDS atomic into the wavefront's own [97] histogram.
// THE 16-BIT RULE. A wavefront counts at most kOrderWavePixels = 1024 pixels of a tile: a ring count is at most 1024 x 24 = 24 576 <
// 2^16, so the halves of a packed word never carry into each other, in a thread or in the wavefront's sum; a bin is at most 1024, a
// tile's word at most 4 x 24 576 = 98 304 (asserted below). The four wavefronts' words are widened where they are
// combined, one table word a thread, and the non-zero words are added to the query's table with 64-bit integer global atomics (the
// caller zeroes the tables on the stream); `pairs` is the tile's pixel count times 8, 16, 24. Integer sums commute: exact and
// byte-identical from call to call.
#include "study_device.h"

namespace musica {

constexpr int kOrderRadius = 3;
constexpr int kOrderWinWords = (kSimTile + 2 * kOrderRadius + 3) / 4;   // words of a staged window row: 70 pixels
constexpr int kOrderWinRows = kSimTile + 2 * kOrderRadius;
constexpr int kOrderLanes = kSimTile / 4;                                // lanes of a tile row, four pixels each
constexpr int kOrderRows = kStudyThreads / kOrderLanes;                  // tile rows of a trip
constexpr int kOrderTrips = kSimTile / kOrderRows;
constexpr int kOrderWavePixels = kSimTile * kSimTile / kStudyWaves;      // what a wavefront counts of a tile
constexpr int kOrderCounts = 4;                                          // same, reversed, flattened, split
constexpr int kOrderWaveWords = kOrderRings * kOrderCounts;              // a wavefront's ring words
static_assert(kOrderWinWords == 18 && kOrderWinRows == 70 && kOrderLanes == 16 && kOrderRows == 16 && kOrderTrips == 4,
              "16 lanes a row, 4 rows a wavefront, 4 trips a tile; a thread's three words end at word 17, its seven rows at row 69");
static_assert(kOrderRings == 3 && kOrderWords == kOrderCounts + 1 && kOrderBins == 2 * (8 + 16 + 24) + 1, "three rings of 8, 16 and 24 neighbours, d = 0 .. 96");
static_assert(kOrderTrips * 4 * 24 == 384 && kOrderWavePixels == 1024 && kOrderWavePixels * 24 == 24576 && kOrderWavePixels * 24 < (1 << 16) &&
                  kStudyWaves * kOrderWavePixels * 24 == 98304,
              "THE 16-BIT RULE: a thread's count and a wavefront's fit half a word, a tile's is far below 2^32");
static_assert(kOrderTableWords == kOrderRings * kOrderWords + kOrderBins && kOrderTableWords <= kStudyThreads, "one table word a thread");

// Byte k = 0 .. 9 of the three words of a window row
__device__ __forceinline__ int order_byte(const uint32_t (&w)[3], int k) { return (int)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu); }

// The masks of pixel i = 0 .. 3 of a thread from its seven rows of three words: lt / gt [ring - 1], 8, 16 and 24 bits from bit 0.
// __builtin_amdgcn_alignbit(m, d, 31) is (m << 1) | (d >> 31): the sign bit of d shifted in.
__device__ __forceinline__ void order_masks(const uint32_t (&w)[2 * kOrderRadius + 1][3], int i, uint32_t (&lt)[kOrderRings], uint32_t (&gt)[kOrderRings]) {
    const int c = order_byte(w[kOrderRadius], i + kOrderRadius);
#pragma unroll
    for (int ring = 1; ring <= kOrderRadius; ring++) {
        const int word = ring - 1;
        lt[word] = gt[word] = 0u;
#pragma unroll
        for (int dy = -ring; dy <= ring; dy++) {
#pragma unroll
            for (int dx = -ring; dx <= ring; dx++) {
                if (max(abs(dx), abs(dy)) != ring) continue;
                const int n = order_byte(w[dy + kOrderRadius], i + kOrderRadius + dx);
                lt[word] = __builtin_amdgcn_alignbit(lt[word], (uint32_t)(n - c), 31);
                gt[word] = __builtin_amdgcn_alignbit(gt[word], (uint32_t)(c - n), 31);
            }
        }
    }
}

__global__ __launch_bounds__(kStudyThreads) void k_order(const OrderQueryDev* __restrict__ qs, unsigned long long* __restrict__ tables) {
    __shared__ uint32_t wa[kOrderWinRows * kOrderWinWords], wb[kOrderWinRows * kOrderWinWords];
    __shared__ uint32_t rings[kStudyWaves][kOrderWaveWords];
    __shared__ uint32_t hist[kStudyWaves][kOrderBins];
    const OrderQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.tiles_x * q.tiles_y) return;   // whole workgroup: the grid is sized for the query with the most tiles
    const TileGeom g = tile_geom(blockIdx.x, q.tiles_x, q.w - 2 * kOrderRadius, q.h - 2 * kOrderRadius);   // of the interior: window pixel (0, 0) is region pixel (x0, y0)
    const int t = threadIdx.x;
    for (int i = t; i < kStudyWaves * kOrderBins; i += kStudyThreads) (&hist[0][0])[i] = 0u;
    stage_windows((const GlobalF32*)q.a + (ptrdiff_t)g.y0 * q.a_pitch + g.x0, q.a_pitch, (const GlobalU8*)q.b + (ptrdiff_t)g.y0 * q.b_pitch + g.x0, q.b_pitch,
                  g.tw + 2 * kOrderRadius, g.th + 2 * kOrderRadius, wa, wb, kOrderWinWords, kOrderWinWords, kOrderWinRows);
    __syncthreads();

    const int lane = t & (kOrderLanes - 1), cx = lane * 4, r = t / kOrderLanes;
    uint32_t* __restrict__ bins = hist[t >> 6];
    uint32_t acc[kOrderWaveWords / 2];   // per ring same | reversed << 16, flattened | split << 16
#pragma unroll
    for (int i = 0; i < kOrderWaveWords / 2; i++) acc[i] = 0u;
    for (int k = 0; k < kOrderTrips; k++) {
        const int ty = k * kOrderRows + r;
        if (ty >= g.th) continue;   // sixteen lanes alike; wave_isum stands behind the loop
        uint32_t a[2 * kOrderRadius + 1][3], b[2 * kOrderRadius + 1][3];
#pragma unroll
        for (int j = 0; j <= 2 * kOrderRadius; j++) {   // rows ty .. ty + 6 <= 69, words lane .. lane + 2 <= 17: inside the staged window
            const int at = (ty + j) * kOrderWinWords + lane;
#pragma unroll
            for (int x = 0; x < 3; x++) {
                a[j][x] = wa[at + x];
                b[j][x] = wb[at + x];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (cx + i >= g.tw) continue;
            uint32_t lta[kOrderRings], gta[kOrderRings], ltb[kOrderRings], gtb[kOrderRings];
            order_masks(a, i, lta, gta);
            order_masks(b, i, ltb, gtb);
            uint32_t d = 0u;
#pragma unroll
            for (int ring = 0; ring < kOrderRings; ring++) {
                const uint32_t sta = lta[ring] | gta[ring], stb = ltb[ring] | gtb[ring];   // strict in a, in b: the bits above a ring's are 0 in both
                const uint32_t same = (uint32_t)__popc((lta[ring] & ltb[ring]) | (gta[ring] & gtb[ring]));
                const uint32_t rev = (uint32_t)__popc((lta[ring] & gtb[ring]) | (gta[ring] & ltb[ring]));
                const uint32_t flat = (uint32_t)__popc(~sta & stb);
                const uint32_t split = (uint32_t)__popc(sta & ~stb);
                acc[2 * ring] += same + (rev << 16);
                acc[2 * ring + 1] += flat + (split << 16);
                d += 2u * rev + flat + split;
            }
            atomicAdd(&bins[d], 1u);   // d <= 96: every mask bit is in one category at most
        }
    }
    wave_isum(acc[0], acc[1], acc[2], acc[3], acc[4], acc[5]);   // all 64 lanes are here; every half at most 24 576
    if (wave_last()) {
#pragma unroll
        for (int i = 0; i < kOrderWaveWords / 2; i++) {
            rings[t >> 6][2 * i] = acc[i] & 0xFFFFu;
            rings[t >> 6][2 * i + 1] = acc[i] >> 16;
        }
    }
    __syncthreads();
    if (t < kOrderTableWords) {   // table word t, the four wavefronts widened to 64 bits
        unsigned long long v = 0ull;
        if (t < kOrderRings * kOrderWords) {
            const int ring = t / kOrderWords, f = t - ring * kOrderWords;
            if (f == 0) v = (unsigned long long)(g.tw * g.th) * (unsigned long long)(8 * (ring + 1));   // pairs: 8, 16, 24 a pixel
            else
                for (int w = 0; w < kStudyWaves; w++) v += rings[w][ring * kOrderCounts + f - 1];
        } else {
            for (int w = 0; w < kStudyWaves; w++) v += hist[w][t - kOrderRings * kOrderWords];
        }
        if (v) atomicAdd((unsigned long long*)((GlobalU64*)tables + q.table + (size_t)t), v);
    }
}

void launch_sim_order(hipStream_t st, const OrderQueryDev* d_qs, int count, int max_tiles, unsigned long long* tables) {
    hipLaunchKernelGGL(k_order, dim3((unsigned)max_tiles, 1, (unsigned)count), dim3(kStudyThreads), 0, st, d_qs, tables);
}

}  // namespace musica
