// kernels_points.hip — the point-response relation of the study (include/musica.h, musica_alter_points / musica_sim_points): defect
// pixels and small clusters inserted into the alteration source on its way into one image of the input buffer, and the two-dimensional
// response around them stacked over all the points of a group, offset by offset. A point is (x, y, R, s, c, group): an integer centre,
// the half-side kPointMinRadius <= R <= kPointMaxRadius of its window |dx|, |dy| <= R (side S = 2R + 1, one R for the whole list), the
// cluster size 1 <= s <= kPointMaxSize (offsets -((s - 1) / 2) .. s / 2 along each axis, all inside the core |dx|, |dy| <= 1), the
// contrast kPointMinContrast <= c <= kPointMaxContrast, c != 0, and a group below kPointMaxGroups. The windows of a list lie inside the
// plane and are pairwise disjoint (the callers check). A list travels packed, PackedPoint = {x | y << 16, R | s << 6 | group << 8 |
// (c - kPointMinContrast) << 12}: a plane side is at most 16384 (musica_create), so 8 bytes say everything.
//
// k_alter_points<V>: harness.insert_points, the insertion body of study_device.h (insert_patches: bin, stream) with the rule: inside a cluster
//   out = min((v (1024 - c) + 512) >> 10, 65535)          v (1024 - c) + 512 <= 65535 * 65536 + 512 < 2^32: exact u32, ONE rounding
// c = 1024 writes 0 (a dead element), c = -64512 multiplies by 64 and saturates (a hot one). The listed square of a point is its core
// (reach 1), which holds every cluster; a chunk that meets one tests its pixels against the cluster's extent.
//   CAPACITY the details' argument. A listed point has its centre within 1 of the tile, per axis x in [-1, 64] in tile coordinates. Its
//            window reaches R >= 4 to either side of the centre, so along each axis it covers at least 9 of the 74 positions -5 .. 68
//            (a centre inside the tile: x - 4 .. x + 4; x = -1: -5 .. 3; x = 64: 60 .. 68). The windows are disjoint, each holds at
//            least 81 of those 74^2 = 5476 pixels: at most floor(5476 / 81) = 67 are listed. (R = 4 points at pitch 9 reach 64.)
//   ROWS     a list may hold 4096 points where a detail list holds 1024, and every workgroup of the body walks the list it is given
//            (measured at 3072^2 with 3969 points: 41.8 us against the details' 9.7 us with 324). So the host orders the list by y and
//            appends one {first, count} entry per tile row (point_rows), and a workgroup hands the body its tile row's range only.
// One launch, 2 B read + 2 B written per pixel, every store width. 1.8 KB of LDS.
//
// k_sim_points<K, P>: harness.point_statistics. OFFSET-STATIONARY stacking: the other list measurements bin within one patch, this one
// accumulates across patches. The host orders the list by group (point_plan: a stable index sort) and cuts each group into chunks of at
// most kPointChunk = 64 points; one workgroup of kStudyThreads takes one chunk. A thread owns the offsets o = t, t + 256, .. < S^2 (K of
// them: 1 for R <= 7, 5 for R <= 17, 17 = ceil(4225 / 256) for the rest) and keeps their three u32 sums, of a, of b and of (a - b)^2,
// in registers across the whole chunk; where in a window they lie (the two plane offsets, whether they are in the core) is worked out
// once, before the points. Consecutive lanes hold consecutive dx of a window row, so a wavefront reads runs of consecutive pixels. Per
// point the centre is fetched on the scalar side (the index is uniform), side a is the graded f32 plane of a batch image quantised with
// out_u8 while it is read (exactly what k_sim reads), side b the slot's u8 plane, both device address space. The loads of P points are
// issued together (P = 4, 2, 1 for K = 1, 5, 17), since the walk is bound by their latency; an offset past S^2 loads the centre and
// counts nowhere. The five per-point sums (window a, b, ssd; core a, b) are reduced over the wavefront with wave_isum and reach one LDS
// slot per wavefront and point, written once; behind the chunk thread j < points adds the four wavefronts' and writes point j's result.
// No per-pixel atomics. The chunk's registers are then added to the group's table [3][S^2] with u32 integer global atomics, consecutive
// lanes on consecutive words; the launcher zeroes the tables on the stream. Integer sums are exact in any order: the results repeat bit
// for bit. Traffic: count S^2 5 B read.
//   WIDTHS   a thread's sums of one offset over a chunk:     kPointChunk 255^2                  (chunk <= 64)
//            a wavefront's and a point's sums over a window: kPointSide^2 255^2 = 274 730 625    (kPointMaxRadius)
//            a table word over a group:                      kPointMax 255^2 = 266 342 400       (kPointMax)
//            all < 2^32 (asserted below): every accumulator on the device is 32 bits wide.
#include <algorithm>
#include <numeric>

#include "study_device.h"

namespace musica {

constexpr int kPointTileCap = 67;   // listed points of one tile: CAPACITY above
constexpr int kPointSide = 2 * kPointMaxRadius + 1;
static_assert(kPointMinRadius >= 4 && ((kSimTile + 10) * (kSimTile + 10)) / ((2 * 4 + 1) * (2 * 4 + 1)) == kPointTileCap,
              "the capacity argument: windows of side >= 9 in the tile grown by 5");
static_assert(kPointMaxSize <= 3, "every cluster lies inside the core, the listed square of reach 1");
static_assert(kPointMaxContrast <= 1024 && 65535ull * (1024 - kPointMinContrast) + 512 < (1ull << 32), "the altered pixel is an exact u32");
static_assert(kPointMaxRadius < (1 << 6) && kPointMaxSize < (1 << 2) && kPointMaxGroups <= (1 << 4) && kPointMaxContrast - kPointMinContrast < (1 << 20),
              "a point packs into PackedPoint");
static_assert((unsigned long long)kPointMax * 255 * 255 < (1ull << 32), "a table word over the largest group fits u32");
static_assert((unsigned long long)kPointSide * kPointSide * 255 * 255 < (1ull << 32), "a point's sums over the largest window fit u32");
static_assert(kPointChunk == 64 && (kPointSide * kPointSide + kStudyThreads - 1) / kStudyThreads == 17, "a chunk's slots, a thread's offsets");
static_assert(kPointWords == 6, "core a, b | window a, b, ssd, pixels");

__device__ __forceinline__ uint32_t point_pixel(uint32_t v, int c) { return min((v * (uint32_t)(1024 - c) + 512u) >> 10, 65535u); }

struct PointInsert {
    typedef PackedPoint Packed;
    struct Entry {
        int x, y, r, c, lo, hi;   // centre in tile coordinates, the core's reach 1, contrast, the cluster's first and last offset
    };
    struct Staged {};
    struct Row {
        bool in;
    };
    static constexpr int kTileCap = kPointTileCap;
    static __device__ __forceinline__ bool meets(const PackedPoint& p, const TileGeom& t, Entry& e) {
        const int s = (int)(p.rsgc >> 6) & 3;
        e = {(int)(p.xy & 0xFFFFu) - t.x0, (int)(p.xy >> 16) - t.y0, 1, (int)(p.rsgc >> 12) + kPointMinContrast, -((s - 1) / 2), s / 2};
        return square_meets(e.x, e.y, 1, t);
    }
    static __device__ __forceinline__ Staged stage(const Entry*, int) { return {}; }
    static __device__ __forceinline__ Row row(const Entry& d, int, int dy, int, const Staged&) { return {dy >= d.lo && dy <= d.hi}; }
    static __device__ __forceinline__ void pixel(const Entry& d, Row& row, int dx, uint16_t& px) {
        if (row.in && dx >= d.lo && dx <= d.hi) px = (uint16_t)point_pixel(px, d.c);
    }
};

// The list as k_alter_points takes it (host): the points ordered by y (the insertion does not depend on the order), then one entry per
// tile row of the plane, {xy: where the points begin that can meet the row (centres in 64 ty - 1 .. 64 ty + 64), rsgc: how many}. A
// list may hold 4096 points and a plane 2304 tiles and more: without the ranges every workgroup would walk the whole list.
void point_rows(std::vector<PackedPoint>& packed, int n) {
    const auto y_of = [](const PackedPoint& p) { return (int)(p.xy >> 16); };
    std::stable_sort(packed.begin(), packed.end(), [&](const PackedPoint& a, const PackedPoint& b) { return y_of(a) < y_of(b); });
    const size_t count = packed.size();
    packed.reserve(count + (size_t)(n + kSimTile - 1) / kSimTile);
    for (int ty = 0; ty < (n + kSimTile - 1) / kSimTile; ty++) {
        const auto lo = std::lower_bound(packed.begin(), packed.begin() + count, ty * kSimTile - 1, [&](const PackedPoint& p, int y) { return y_of(p) < y; });
        const auto hi = std::lower_bound(packed.begin(), packed.begin() + count, ty * kSimTile + kSimTile + 1, [&](const PackedPoint& p, int y) { return y_of(p) < y; });
        packed.push_back({(uint32_t)(lo - packed.begin()), (uint32_t)(hi - lo)});
    }
}

// n % V == 0 and both planes aligned to 2 V bytes; points: point_rows' list of `count` points and the tile rows' entries behind them
template <int V>
__global__ __launch_bounds__(kStudyThreads) void k_alter_points(const uint16_t* __restrict__ src, uint16_t* __restrict__ out, int n,
                                                                const PackedPoint* __restrict__ points, int count) {
    const int tiles = (n + kSimTile - 1) / kSimTile;
    const PackedPoint row = points[count + (int)blockIdx.x / tiles];
    insert_patches<PointInsert, V>(src, out, n, points + row.xy, (int)row.rsgc);
}

void launch_alter_points(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const PackedPoint* d_points, int count) {
    launch_insert([&](auto v, dim3 grid, dim3 block) { hipLaunchKernelGGL((k_alter_points<decltype(v)::value>), grid, block, 0, st, src, out, n, d_points, count); },
                  src, out, n);
}

// The launch plan of a list: plan[0 .. count) the points' indices ordered by group (stable: inside a group the list's order), then three
// words per chunk: where it starts in that order, its points (1 .. kPointChunk) and its group. Returns the chunks, at most
// kPointMaxChunks. A group without points has no chunk.
int point_plan(const PackedPoint* points, int count, std::vector<uint32_t>& plan) {
    const auto group = [&](uint32_t i) { return (points[i].rsgc >> 8) & 0xFu; };
    plan.resize((size_t)count);
    std::iota(plan.begin(), plan.end(), 0u);
    std::stable_sort(plan.begin(), plan.end(), [&](uint32_t i, uint32_t j) { return group(i) < group(j); });
    int chunks = 0;
    for (int first = 0; first < count;) {
        const uint32_t g = group(plan[first]);
        int end = first;
        while (end < count && group(plan[end]) == g) end++;
        for (; first < end; first += kPointChunk, chunks++) {
            plan.push_back((uint32_t)first);
            plan.push_back((uint32_t)std::min(kPointChunk, end - first));
            plan.push_back(g);
        }
        first = end;
    }
    return chunks;
}

// a: the graded f32 plane at output pixel (0, 0) (the margin skipped), b: the slot's plane; plan: point_plan's words; results: count x
// kPointWords u64; tables: [groups][3][S^2] u32, zeroed. S^2 <= K * kStudyThreads.
template <int K, int P>
__global__ __launch_bounds__(kStudyThreads) void k_sim_points(const float* __restrict__ a_plane, int a_pitch, const uint8_t* __restrict__ b_plane, int b_pitch,
                                                              const PackedPoint* __restrict__ points, const uint32_t* __restrict__ plan, int count, int radius,
                                                              unsigned long long* __restrict__ results, uint32_t* __restrict__ tables) {
    __shared__ uint32_t slots[kStudyWaves][kPointChunk][5];
    const GlobalF32* pa = (const GlobalF32*)a_plane;
    const GlobalU8* pb = (const GlobalU8*)b_plane;
    const int side = 2 * radius + 1, side2 = side * side;
    const uint32_t* chunk = plan + count + 3 * blockIdx.x;
    const int first = (int)chunk[0], m = (int)chunk[1], group = (int)chunk[2];
    const int wave = threadIdx.x >> 6;

    // a thread's offsets: where they lie in a window, once for the whole chunk. One past the window sits on the centre and is not live.
    int off_a[K], off_b[K];
    uint32_t live = 0u, core = 0u;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int o = k * kStudyThreads + (int)threadIdx.x;
        off_a[k] = off_b[k] = 0;
        if (o < side2) {
            const int row = o / side, dy = row - radius, dx = o - row * side - radius;
            off_a[k] = dy * a_pitch + dx;
            off_b[k] = dy * b_pitch + dx;
            live |= 1u << k;
            if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1) core |= 1u << k;
        }
    }

    uint32_t sa[K] = {}, sb[K] = {}, sd[K] = {};
    for (int j0 = 0; j0 < m; j0 += P) {
        uint32_t a[P][K], b[P][K];
        // P points' loads together. A point past the chunk is the chunk's last one again, and counted nowhere.
#pragma unroll
        for (int q = 0; q < P; q++) {
            const PackedPoint p = points[plan[first + min(j0 + q, m - 1)]];   // uniform: the scalar side
            const int cx = (int)(p.xy & 0xFFFFu), cy = (int)(p.xy >> 16);
            const GlobalF32* ca = pa + ((size_t)cy * a_pitch + cx);
            const GlobalU8* cb = pb + ((size_t)cy * b_pitch + cx);
#pragma unroll
            for (int k = 0; k < K; k++) {
                a[q][k] = out_u8(ca[off_a[k]]);
                b[q][k] = cb[off_b[k]];
            }
        }
#pragma unroll
        for (int q = 0; q < P; q++) {
            const uint32_t there = j0 + q < m ? live : 0u;
            uint32_t wa = 0u, wb = 0u, wd = 0u, ka = 0u, kb = 0u;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const bool on = (there >> k) & 1u, in_core = (core >> k) & 1u;
                const uint32_t va = on ? a[q][k] : 0u, vb = on ? b[q][k] : 0u;
                const uint32_t diff = va > vb ? va - vb : vb - va, d2 = diff * diff;
                sa[k] += va;
                sb[k] += vb;
                sd[k] += d2;
                wa += va;
                wb += vb;
                wd += d2;
                ka += in_core ? va : 0u;
                kb += in_core ? vb : 0u;
            }
            wave_isum(wa, wb, wd, ka, kb);
            if (wave_last() && j0 + q < m) {
                uint32_t* s = slots[wave][j0 + q];
                s[0] = ka;
                s[1] = kb;
                s[2] = wa;
                s[3] = wb;
                s[4] = wd;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < m) {
        // musica_sim_point_result: core_sum_a, core_sum_b, win_sum_a, win_sum_b, win_ssd, win_pixels
        unsigned long long* o = results + (size_t)plan[first + threadIdx.x] * kPointWords;
        for (int i = 0; i < 5; i++) {
            uint32_t v = slots[0][threadIdx.x][i];
            for (int w = 1; w < kStudyWaves; w++) v += slots[w][threadIdx.x][i];
            o[i] = v;
        }
        o[5] = (unsigned long long)side2;
    }
    uint32_t* table = tables + (size_t)group * 3 * side2;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int o = k * kStudyThreads + (int)threadIdx.x;
        if (o < side2) {
            __hip_atomic_fetch_add(table + o, sa[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(table + side2 + o, sb[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(table + 2 * side2 + o, sd[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

void launch_sim_points(hipStream_t st, const float* a_plane, int a_pitch, const uint8_t* b_plane, int b_pitch, const PackedPoint* d_points, int count, int radius,
                       int groups, const uint32_t* plan, int chunks, uint32_t* d_plan, unsigned long long* results, uint32_t* tables) {
    const int side2 = (2 * radius + 1) * (2 * radius + 1);
    (void)hipMemsetAsync(tables, 0, (size_t)groups * 3 * side2 * sizeof(uint32_t), st);
    (void)hipMemcpyAsync(d_plan, plan, ((size_t)count + 3 * (size_t)chunks) * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    const dim3 grid((unsigned)chunks), block(kStudyThreads);
    if (side2 <= kStudyThreads)
        hipLaunchKernelGGL((k_sim_points<1, 4>), grid, block, 0, st, a_plane, a_pitch, b_plane, b_pitch, d_points, d_plan, count, radius, results, tables);
    else if (side2 <= 5 * kStudyThreads)
        hipLaunchKernelGGL((k_sim_points<5, 2>), grid, block, 0, st, a_plane, a_pitch, b_plane, b_pitch, d_points, d_plan, count, radius, results, tables);
    else
        hipLaunchKernelGGL((k_sim_points<17, 1>), grid, block, 0, st, a_plane, a_pitch, b_plane, b_pitch, d_points, d_plan, count, radius, results, tables);
}

}  // namespace musica
