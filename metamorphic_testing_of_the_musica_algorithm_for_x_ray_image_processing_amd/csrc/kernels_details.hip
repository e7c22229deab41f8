// kernels_details.hip — the contrast-detail relation of the study (include/musica.h, musica_alter_details / musica_sim_details): discs
// inserted into the alteration source on its way into one image of the input buffer, and the per-detail masked sums of an output
// against a reference slot. A detail is (x, y, r, c): an integer centre, 1 <= r <= kDetailMaxRadius, 1 <= |c| <= kDetailMaxContrast;
// with d2 = (px - x)^2 + (py - y)^2 its zones are the disc d2 <= r^2, the ring (r + 2)^2 <= d2 <= (2r + 2)^2 and the box |px - x|,
// |py - y| <= 2r + 2 (side 4r + 5). The boxes of a list lie inside the plane and are pairwise disjoint (the callers check), so a pixel
// belongs to at most one disc and to at most one box. A list travels packed, PackedDetail = {x | y << 16, r | (c + 512) << 8}: a plane
// side is at most 16384 (musica_create), so 8 bytes say everything.
//
// k_alter_details<V>: harness.insert_details, the insertion body of study_device.h (insert_patches: bin, stream) with the rule: inside a disc
//   out = min((v (1024 - c) + 512) >> 10, 65535)          v (1024 - c) + 512 <= 65535 * 1536 + 512 < 2^32: exact u32, ONE rounding
// The listed square of a detail is its disc's bounding square (side 2r + 1), and only the chunks that meet one compute d2 per pixel.
//   CAPACITY A listed detail has its centre within r of the tile, per axis x in [-r, 63 + r] in tile coordinates. Its box
//            reaches 2r + 2 >= 4 to either side of the centre, so along each axis it covers at least 9 of the 74 positions -5 .. 68
//            (a centre inside the tile: x - 4 .. x + 4; one left of it: from -5 or further left up to x + 2r + 2 >= r + 2 >= 3; right
//            likewise). The boxes are disjoint, each holds at least 81 of those 74^2 = 5476 pixels: at most floor(5476 / 81) = 67 are
//            listed. (r = 1 details at pitch 9 reach 64.)
// 1.1 KB of LDS.
//
// k_sim_details: harness.detail_statistics. One workgroup of 256 threads per detail; side a is the graded f32 plane of a batch image
// quantised with out_u8 while it is read (exactly what k_sim reads), side b the slot's u8 plane, the detail in the coordinates of the
// cropped output plane. The wavefronts take the box's rows round-robin and the lanes its columns in steps of 64, so a wavefront reads
// runs of consecutive pixels; a lane loads four of its rows together, since the walk is bound by the latency of its loads. A lane
// keeps 13 partial sums in u32: n, sum a, sum b, sum a^2, sum b^2, sum a b of the disc and of the ring, and the box's sum (a - b)^2.
// It sees at most ceil(side / 4) rows x ceil(side / 64) columns = 66 * 5 = 330 pixels of the largest box, and 330 * 255^2 < 2^32
// (asserted below on the limits). The partials are widened to u64, reduced in the study's ONE order (wave_sum, then WaveSlots:
// study_device.h) and written by thread 0: no atomics, so the results repeat bit for bit.
#include "study_device.h"

namespace musica {

constexpr int kDetailThreads = 256;
constexpr int kDetailTileCap = 67;   // listed details of one tile: CAPACITY above
static_assert(kDetailThreads == kStudyThreads, "k_sim_details reduces over the study's workgroup");
static_assert(kDetailMaxRadius >= 1 && ((kSimTile + 10) * (kSimTile + 10)) / 81 == kDetailTileCap, "the capacity argument: boxes of side >= 9 in the tile grown by 5");
static_assert(kDetailMaxContrast <= 512 && 65535ull * (1024 + kDetailMaxContrast) + 512 < (1ull << 32), "the attenuated pixel is an exact u32");
static_assert(kDetailMaxRadius < 256 && kDetailMaxContrast + 512 < (1 << 24), "a detail packs into PackedDetail");
constexpr unsigned long long kDetailBoxSide = 4ull * kDetailMaxRadius + 5;
static_assert(((kDetailBoxSide + kStudyWaves - 1) / kStudyWaves) * ((kDetailBoxSide + 63) / 64) * 255ull * 255ull < (1ull << 32),
              "a lane's partial sums over the largest box fit u32");

__device__ __forceinline__ uint32_t detail_pixel(uint32_t v, int c) { return min((v * (uint32_t)(1024 - c) + 512u) >> 10, 65535u); }

struct DetailInsert {
    typedef PackedDetail Packed;
    struct Entry {
        int x, y, r, c;   // centre in tile coordinates, radius, contrast
    };
    struct Staged {};
    struct Row {
        int r2, dy2;
    };
    static constexpr int kTileCap = kDetailTileCap;
    static __device__ __forceinline__ bool meets(const PackedDetail& p, const TileGeom& t, Entry& e) {
        e = {(int)(p.xy & 0xFFFFu) - t.x0, (int)(p.xy >> 16) - t.y0, (int)(p.rc & 0xFFu), (int)(p.rc >> 8) - 512};
        return square_meets(e.x, e.y, e.r, t);
    }
    static __device__ __forceinline__ Staged stage(const Entry*, int) { return {}; }
    static __device__ __forceinline__ Row row(const Entry& d, int, int dy, int, const Staged&) { return {d.r * d.r, dy * dy}; }
    static __device__ __forceinline__ void pixel(const Entry& d, Row& row, int dx, uint16_t& px) {
        if (dx * dx + row.dy2 <= row.r2) px = (uint16_t)detail_pixel(px, d.c);
    }
};

// n % V == 0 and both planes aligned to 2 V bytes
template <int V>
__global__ __launch_bounds__(kDetailThreads) void k_alter_details(const uint16_t* __restrict__ src, uint16_t* __restrict__ out, int n,
                                                                   const PackedDetail* __restrict__ details, int count) {
    insert_patches<DetailInsert, V>(src, out, n, details, count);
}

void launch_alter_details(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const PackedDetail* d_details, int count) {
    launch_insert([&](auto v, dim3 grid, dim3 block) { hipLaunchKernelGGL((k_alter_details<decltype(v)::value>), grid, block, 0, st, src, out, n, d_details, count); },
                  src, out, n);
}

constexpr int kDetailSums = 13;   // disc n, a, b, aa, bb, ab | ring the same six | box ssd
constexpr int kDetailRows = 4;    // box rows of one column that a lane loads together

// a: the graded f32 plane at output pixel (0, 0) (the margin skipped), b: the slot's plane; out: count x kDetailWords u64
__global__ __launch_bounds__(kDetailThreads) void k_sim_details(const float* __restrict__ a_plane, int a_pitch, const uint8_t* __restrict__ b_plane,
                                                                 int b_pitch, const PackedDetail* __restrict__ details,
                                                                 unsigned long long* __restrict__ out) {
    __shared__ WaveSlots<unsigned long long, kDetailSums> slots;
    const GlobalF32* pa = (const GlobalF32*)a_plane;
    const GlobalU8* pb = (const GlobalU8*)b_plane;
    const PackedDetail p = details[blockIdx.x];
    const int cx = (int)(p.xy & 0xFFFFu), cy = (int)(p.xy >> 16), r = (int)(p.rc & 0xFFu);
    const int ro = 2 * r + 2, side = 2 * ro + 1;
    const int disc2 = r * r, ring_lo = (r + 2) * (r + 2), ring_hi = ro * ro;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t s[kDetailSums] = {};
    // kDetailRows rows of a lane's column at a time: their loads are issued together, or the walk would wait for one pixel after the
    // other. A row past the box is loaded at the box's last row and counted nowhere.
    for (int row0 = wave; row0 < side; row0 += kStudyWaves * kDetailRows) {
        for (int col = lane; col < side; col += 64) {
            const int dx = col - ro, x = cx + dx;
            uint32_t a[kDetailRows], b[kDetailRows];
#pragma unroll
            for (int k = 0; k < kDetailRows; k++) {
                const int y = cy + min(row0 + k * kStudyWaves, side - 1) - ro;
                a[k] = out_u8(pa[(size_t)y * a_pitch + x]);
                b[k] = pb[(size_t)y * b_pitch + x];
            }
#pragma unroll
            for (int k = 0; k < kDetailRows; k++) {
                const int row = row0 + k * kStudyWaves, dy = row - ro;
                const uint32_t live = row < side ? 1u : 0u;
                const int d2 = dx * dx + dy * dy;
                const uint32_t diff = a[k] > b[k] ? a[k] - b[k] : b[k] - a[k];
                s[12] += live * diff * diff;
                const uint32_t in_disc = d2 <= disc2 ? live : 0u, in_ring = (d2 >= ring_lo && d2 <= ring_hi) ? live : 0u;
                const uint32_t aa = a[k] * a[k], bb = b[k] * b[k], ab = a[k] * b[k];
                s[0] += in_disc;
                s[1] += in_disc * a[k];
                s[2] += in_disc * b[k];
                s[3] += in_disc * aa;
                s[4] += in_disc * bb;
                s[5] += in_disc * ab;
                s[6] += in_ring;
                s[7] += in_ring * a[k];
                s[8] += in_ring * b[k];
                s[9] += in_ring * aa;
                s[10] += in_ring * bb;
                s[11] += in_ring * ab;
            }
        }
    }
    unsigned long long w[kDetailSums];
#pragma unroll
    for (int i = 0; i < kDetailSums; i++) w[i] = s[i];
    wave_sum(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12]);
    if (wave_leader()) slots.put(w);
    __syncthreads();
    if (threadIdx.x == 0) {
        // musica_sim_detail_result: n[2], sum_a[2], sum_b[2], sum_aa[2], sum_bb[2], sum_ab[2] (disc, ring), box_ssd, box_pixels
        unsigned long long* o = out + (size_t)blockIdx.x * kDetailWords;
        for (int q = 0; q < 6; q++) {
            o[2 * q] = slots.sum(q);
            o[2 * q + 1] = slots.sum(6 + q);
        }
        o[12] = slots.sum(12);
        o[13] = (unsigned long long)side * side;
    }
}

void launch_sim_details(hipStream_t st, const float* a_plane, int a_pitch, const uint8_t* b_plane, int b_pitch, const PackedDetail* d_details, int count,
                        unsigned long long* out) {
    hipLaunchKernelGGL(k_sim_details, dim3((unsigned)count), dim3(kDetailThreads), 0, st, a_plane, a_pitch, b_plane, b_pitch, d_details, out);
}

}  // namespace musica
