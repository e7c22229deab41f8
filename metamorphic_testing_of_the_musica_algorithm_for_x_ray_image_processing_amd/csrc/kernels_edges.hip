// kernels_edges.hip — the edge-response relation of the study (include/musica.h, musica_alter_edges / musica_sim_edges): slanted edges
// inserted into the alteration source on its way into one image of the input buffer, and the edge-spread tables of an output against a
// reference slot. An edge is (x, y, h, p, q, o, c): an integer centre, a half-side kEdgeMinHalf <= h <= kEdgeMaxHalf, a slope p / q
// (1 <= p < q, kEdgeMinQ <= q <= kEdgeMaxQ, lowest terms), an orientation o = 0 .. 3, 1 <= |c| <= kEdgeMaxContrast. With dx = px - x,
// dy = py - y the profile and along-edge coordinates (u, v) are (dx, dy), (dy, dx), (-dx, dy), (-dy, dx) for o = 0 .. 3 and the signed
// numerator is s = q u - p v, which is LINEAR in the pixel: s = A dx + B dy with (A, B) = (q, -p), (-p, q), (-q, -p), (-p, -q)
// (edge_axes). The plate |dx|, |dy| <= 2h (side 4h + 1) is inserted, the region |dx|, |dy| <= h (side 2h + 1) measured. The plates of
// a list lie inside the plane and are pairwise disjoint (the callers check), so a pixel belongs to at most one plate. A list travels
// packed, PackedEdge (launchers.h): a plane side is at most 16384.
//
// k_alter_edges<V>: harness.insert_edges, the insertion body of study_device.h (insert_patches: bin, stream) with the rule: inside a
// plate, with m = clamp(2s + q, 0, 2q),
//   out = min((v (2048 q - c m) + 1024 q) div (2048 q), 65535)      v (2048 q - c m) + 1024 q <= 65535 * (2048 * 16 + 512 * 32) + 16384
//                                                                   < 2^32: exact u32, ONE rounding (asserted below on the limits)
// m = 0 (s <= -q / 2: the bare side) is v itself and is not computed; m = 2q (the absorber's side) is
// detail_pixel's min((v (1024 - c) + 512) >> 10, 65535), the same number without a division (2q cancels); only the pixels of the
// transition band 0 < m < 2q divide, as (x >> 11) / q in u32: floor(floor(x / 2048) / q) = floor(x / (2048 q)).
// The listed square of an edge is its plate, and only the chunks that meet one compute s per pixel.
//   CAPACITY A plate has side 4h + 1 >= 33. Along an axis, in tile coordinates, a listed plate is an interval of at least 33
//            positions that meets 0 .. 63, so it covers at least 33 of the 128 positions -32 .. 95: all of itself where it starts at
//            -32 or later and ends at 95 or sooner, else -32 .. its end >= 0, or its start <= 63 .. 95. The plates are disjoint and
//            each holds at least 33^2 = 1089 of those 128^2 = 16384 pixels: at most floor(16384 / 1089) = 15 are listed. (h = 8 plates
//            at pitch 33 reach 9: three to an axis.)
// 0.5 KB of LDS.
//
// k_sim_edges: harness.edge_statistics. One workgroup of 256 threads per edge; side a is the graded f32 plane of a batch image quantised
// with out_u8 while it is read (exactly what k_sim reads), side b the slot's u8 plane, the edge in the coordinates of the cropped output
// plane. Every pixel of the region adds 1, a, b and a^2 into bin floor(4 s / q) + B of the edge's table, B = ceil(4 (q + p) h / q),
// 2B + 1 <= 16h - 1 <= 2047 bins. The table is privatised in LDS as u32 [4][kEdgeBinsMax] = 32 KiB and filled with LDS integer atomics
// (ds_add_u32, no return): integer addition commutes, so the table is exact and repeats from call to call whatever order the
// wavefronts arrive in (kernels_joint.hip's argument). A bin holds at most 2h + 1 = 257 pixels, 257 * 255^2 < 2^32.
//   walk     the wavefronts take the region's rows round-robin and the lanes its columns in steps of 64, so a wavefront reads runs of
//            consecutive pixels; a lane loads kEdgeRows of its rows together, since the walk is bound by the latency of its loads.
//            Consecutive lanes are 4 bins apart where the row runs along the profile (o = 0, 2) and 4 p / q < 4 bins apart where it
//            runs along the edge, so at most ceil(q / 4p) + 1 <= 5 lanes of a wavefront meet in one bin.
//   no division per pixel   4s is linear, so the bin is carried as (k, rem) with 4s = k q + rem, 0 <= rem < q: a step of 64 columns adds
//            the constants floor(256 A / q) and 256 A mod q, a step of 16 rows floor(64 B / q) and 64 B mod q, each with one carry
//            (k_zoom's walk). A lane divides four times at the start, for the first pixel of each of its kEdgeRows row phases.
//   roi_ssd  u32 per lane (at most 65 rows x 5 columns = 325 pixels, 325 * 255^2 < 2^32: asserted below), then the study's ONE
//            reduction order (wave_sum, then WaveSlots: study_device.h).
// After a barrier the workgroup writes the table's 4 x (2B + 1) words to its place in the flat output with coalesced stores and
// thread 0 the four u64 of the result. No global atomics.
#include "study_device.h"

namespace musica {

constexpr int kEdgeThreads = 256;
constexpr int kEdgeTileCap = 15;   // listed plates of one tile: CAPACITY above
constexpr int kEdgeMinPlate = 4 * kEdgeMinHalf + 1;
static_assert(kEdgeThreads == kStudyThreads, "k_sim_edges reduces over the study's workgroup");
static_assert(kEdgeMinPlate == 33 && ((kSimTile + 2 * (kEdgeMinPlate - 1)) * (kSimTile + 2 * (kEdgeMinPlate - 1))) / (kEdgeMinPlate * kEdgeMinPlate) == kEdgeTileCap,
              "the capacity argument: plates of side >= 33 in the tile grown by 32");
static_assert(65535ull * (2048ull * kEdgeMaxQ + (unsigned long long)kEdgeMaxContrast * 2 * kEdgeMaxQ) + 1024ull * kEdgeMaxQ < (1ull << 32),
              "the attenuated pixel is an exact u32");
static_assert(kEdgeMaxContrast <= 1024, "2048 q - c m >= 0: c m <= 1024 * 2q");
static_assert(16 * kEdgeMaxHalf - 1 < kEdgeBinsMax, "2B + 1 <= 16h - 1 bins fit the LDS table");
static_assert((2ull * kEdgeMaxHalf + 1) * 255 * 255 < (1ull << 32), "a bin's sums fit u32: at most 2h + 1 pixels");
constexpr int kEdgeRows = 4;       // region rows of one column that a lane loads together
constexpr unsigned long long kEdgeSide = 2ull * kEdgeMaxHalf + 1;
static_assert(((kEdgeSide + kStudyWaves - 1) / kStudyWaves) * ((kEdgeSide + 63) / 64) * 255ull * 255ull < (1ull << 32), "a lane's roi_ssd over the largest region fits u32");
static_assert(kEdgeMaxHalf < 256 && kEdgeMaxQ < 256, "an edge packs into PackedEdge");

struct EdgeAxes {
    int a, b;   // s = a dx + b dy
};
__device__ __forceinline__ EdgeAxes edge_axes(int p, int q, int o) {
    return o == 0 ? EdgeAxes{q, -p} : o == 1 ? EdgeAxes{-p, q} : o == 2 ? EdgeAxes{-q, -p} : EdgeAxes{-p, -q};
}

// 0 < m <= 2q
__device__ __forceinline__ uint32_t edge_pixel(uint32_t v, int c, int q, int m) {
    if (m == 2 * q) return min((v * (uint32_t)(1024 - c) + 512u) >> 10, 65535u);
    return min(((v * (uint32_t)(2048 * q - c * m) + 1024u * (uint32_t)q) >> 11) / (uint32_t)q, 65535u);
}

struct EdgeInsert {
    typedef PackedEdge Packed;
    struct Entry {
        int x, y, r, a, b, q, c;   // centre in tile coordinates, the plate's reach 2h, s = a dx + b dy, q, contrast
    };
    struct Staged {};
    typedef int Row;               // b dy
    static constexpr int kTileCap = kEdgeTileCap;
    static __device__ __forceinline__ bool meets(const PackedEdge& e, const TileGeom& t, Entry& d) {
        const int x = (int)(e.xy & 0xFFFFu) - t.x0, y = (int)(e.xy >> 16) - t.y0, r = 2 * (int)(e.hpqo & 0xFFu);
        if (!square_meets(x, y, r, t)) return false;
        const int p = (int)((e.hpqo >> 8) & 0xFFu), q = (int)((e.hpqo >> 16) & 0xFFu);
        const EdgeAxes ax = edge_axes(p, q, (int)(e.hpqo >> 24));
        d = {x, y, r, ax.a, ax.b, q, e.c};
        return true;
    }
    static __device__ __forceinline__ Staged stage(const Entry*, int) { return {}; }
    static __device__ __forceinline__ Row row(const Entry& d, int, int dy, int, const Staged&) { return d.b * dy; }
    static __device__ __forceinline__ void pixel(const Entry& d, Row& row, int dx, uint16_t& px) {
        const int cover = min(max(2 * (d.a * dx + row) + d.q, 0), 2 * d.q);
        if (dx >= -d.r && dx <= d.r && cover > 0) px = (uint16_t)edge_pixel(px, d.c, d.q, cover);
    }
};

// n % V == 0 and both planes aligned to 2 V bytes
template <int V>
__global__ __launch_bounds__(kEdgeThreads) void k_alter_edges(const uint16_t* __restrict__ src, uint16_t* __restrict__ out, int n,
                                                               const PackedEdge* __restrict__ edges, int count) {
    insert_patches<EdgeInsert, V>(src, out, n, edges, count);
}

void launch_alter_edges(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const PackedEdge* d_edges, int count) {
    launch_insert([&](auto v, dim3 grid, dim3 block) { hipLaunchKernelGGL((k_alter_edges<decltype(v)::value>), grid, block, 0, st, src, out, n, d_edges, count); },
                  src, out, n);
}

// floor(t / q) for q > 0 and any t
__device__ __forceinline__ int floor_div(int t, int q) {
    const int d = t / q;
    return d - (t - d * q < 0 ? 1 : 0);
}

// a: the graded f32 plane at output pixel (0, 0) (the margin skipped), b: the slot's plane; results: count x kEdgeWords u64; tables:
// edge i's 4 x bins_i u32 at its PackedEdge::table
__global__ __launch_bounds__(kEdgeThreads) void k_sim_edges(const float* __restrict__ a_plane, int a_pitch, const uint8_t* __restrict__ b_plane,
                                                             int b_pitch, const PackedEdge* __restrict__ edges,
                                                             unsigned long long* __restrict__ results, uint32_t* __restrict__ tables) {
    __shared__ uint32_t table[4][kEdgeBinsMax];
    __shared__ WaveSlots<unsigned long long> slots;
    const GlobalF32* pa = (const GlobalF32*)a_plane;
    const GlobalU8* pb = (const GlobalU8*)b_plane;
    const PackedEdge e = edges[blockIdx.x];
    const int cx = (int)(e.xy & 0xFFFFu), cy = (int)(e.xy >> 16), h = (int)(e.hpqo & 0xFFu);
    const int p = (int)((e.hpqo >> 8) & 0xFFu), q = (int)((e.hpqo >> 16) & 0xFFu);
    const EdgeAxes ax = edge_axes(p, q, (int)(e.hpqo >> 24));
    const int big = (4 * (q + p) * h + q - 1) / q, bins = 2 * big + 1, side = 2 * h + 1;
    for (int i = threadIdx.x; i < bins; i += kEdgeThreads) table[0][i] = table[1][i] = table[2][i] = table[3][i] = 0u;
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // 4s = k q + rem: what 64 columns and what kStudyWaves * kEdgeRows rows add to it
    const int col_k = floor_div(4 * 64 * ax.a, q), col_rem = 4 * 64 * ax.a - col_k * q;
    const int row_k = floor_div(4 * kStudyWaves * kEdgeRows * ax.b, q), row_rem = 4 * kStudyWaves * kEdgeRows * ax.b - row_k * q;
    int row_bin[kEdgeRows], row_left[kEdgeRows];   // the bin (index k + B) and remainder of pixel (column `lane`, row row0 + j kStudyWaves)
#pragma unroll
    for (int j = 0; j < kEdgeRows; j++) {
        const int s4 = 4 * (ax.a * (lane - h) + ax.b * (wave + j * kStudyWaves - h));
        const int k = floor_div(s4, q);
        row_bin[j] = k + big;
        row_left[j] = s4 - k * q;
    }
    uint32_t ssd = 0u;
    // kEdgeRows rows of a lane's column at a time: their loads are issued together. A row past the region is loaded at the region's
    // last row and counted nowhere.
    for (int row0 = wave; row0 < side; row0 += kStudyWaves * kEdgeRows) {
        int bin[kEdgeRows], left[kEdgeRows];
#pragma unroll
        for (int j = 0; j < kEdgeRows; j++) {
            bin[j] = row_bin[j];
            left[j] = row_left[j];
        }
        for (int col = lane; col < side; col += 64) {
            const int x = cx - h + col;
            uint32_t a[kEdgeRows], b[kEdgeRows];
#pragma unroll
            for (int j = 0; j < kEdgeRows; j++) {
                const int y = cy - h + min(row0 + j * kStudyWaves, side - 1);
                a[j] = out_u8(pa[(size_t)y * a_pitch + x]);
                b[j] = pb[(size_t)y * b_pitch + x];
            }
#pragma unroll
            for (int j = 0; j < kEdgeRows; j++) {
                // a live pixel's bin is 0 .. 2B by the contract's arithmetic; the second test keeps a slip inside the table
                if (row0 + j * kStudyWaves < side && (unsigned)bin[j] < (unsigned)bins) {
                    const uint32_t diff = a[j] > b[j] ? a[j] - b[j] : b[j] - a[j];
                    ssd += diff * diff;
                    atomicAdd(&table[0][bin[j]], 1u);
                    atomicAdd(&table[1][bin[j]], a[j]);
                    atomicAdd(&table[2][bin[j]], b[j]);
                    atomicAdd(&table[3][bin[j]], a[j] * a[j]);
                }
                bin[j] += col_k;
                left[j] += col_rem;
                if (left[j] >= q) {
                    left[j] -= q;
                    bin[j]++;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kEdgeRows; j++) {
            row_bin[j] += row_k;
            row_left[j] += row_rem;
            if (row_left[j] >= q) {
                row_left[j] -= q;
                row_bin[j]++;
            }
        }
    }
    unsigned long long w = ssd;
    wave_sum(w);
    if (wave_leader()) slots.put(w);
    __syncthreads();   // the table is complete, the wavefronts' sums are in place
    uint32_t* o = tables + e.table;
    for (int j = 0; j < 4; j++)
        for (int i = threadIdx.x; i < bins; i += kEdgeThreads) o[j * bins + i] = table[j][i];
    if (threadIdx.x == 0) {
        // musica_sim_edge_result: roi_ssd, roi_pixels, table_offset, bins
        unsigned long long* r = results + (size_t)blockIdx.x * kEdgeWords;
        r[0] = slots.sum();
        r[1] = (unsigned long long)side * side;
        r[2] = e.table;
        r[3] = (unsigned long long)bins;
    }
}

void launch_sim_edges(hipStream_t st, const float* a_plane, int a_pitch, const uint8_t* b_plane, int b_pitch, const PackedEdge* d_edges, int count,
                      unsigned long long* results, uint32_t* tables) {
    hipLaunchKernelGGL(k_sim_edges, dim3((unsigned)count), dim3(kEdgeThreads), 0, st, a_plane, a_pitch, b_plane, b_pitch, d_edges, results, tables);
}

}  // namespace musica
