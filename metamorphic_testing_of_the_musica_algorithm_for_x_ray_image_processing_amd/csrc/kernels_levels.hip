// kernels_levels.hip — the tone-table relation of the study (include/musica.h, musica_alter_lut / musica_sim_levels): a 65536-entry
// table applied to the alteration source on its way into one image of the input buffer, and the exact sums of a comparison of an
// output against a reference slot, kept apart by the level of the INPUT pixel: the characteristic curve of the chain, before and after.
//
// k_alter_lut<V>: harness.apply_lut, out = lut[src]. ONE launch, 2 B read + 2 B written per pixel. The map is point-wise, so the dense
// n x n plane is a flat run of n^2 pixels: a thread moves chunks of V consecutive pixels (study_device.h's pixel words, the alignment
// test taken on n^2 instead of n: V = 8, one 16-byte access, where n^2 % 8 == 0 and both planes are 16-byte aligned, else 2 under the
// same condition for 4 bytes, else single pixels: images of a batch with odd n^2 start on a 2-byte boundary only); consecutive lanes
// take consecutive chunks, a thread kLutChunks of them at a time, all loaded before the first lookup. V lookups per chunk.
// WHERE THE TABLE LIVES: in LDS, all 128 KiB of it. At most one workgroup of 1024 threads per CU (kLutBlocks = 256, fewer for a small
// plane) copies the table with eight 16-byte loads a thread, its first chunks already in flight, and strides over the plane; a lookup
// is a ds_read_u16. The staging is 128 KiB of L2 reads a workgroup, 32 MiB a launch, more bytes than a 2048^2 plane moves, but they
// come from the L2 (the table fits an XCD's 4 MiB 32 times) at 16 bytes a lane, while the plain alternative, one 2-byte global load
// per pixel through L1, makes a wavefront's load touch up to 64 lines of a table four times the L1. MEASURED both ways (DESIGN.md
// section 4): staged 17.2 us against 24.3 us at 3072^2 and faster at every side from 512 up; the global form was not kept.
// Nothing outside the two planes and the table is read, nothing outside `out` written; the planes must not overlap.
//
// k_sim_levels: harness.level_statistics. Every query owns blockIdx.z, as in k_joint. Side a is the graded f32 plane of a batch image
// quantised with out_u8 while it is read (load_quant4: exactly what k_sim reads), side b the slot's u8 plane, and the class of a pixel
// is the alteration source at side a's coordinates (margin added by the caller) >> shift: 4 + 1 + 2 bytes per pixel, once. A class's
// six words are n, sum a, sum b, sum (a - b)^2, sum a^2, sum b^2.
//   * A workgroup of 1024 threads privatises a query's whole table in LDS, PACKED: per class one u64 of n (16 bits), sum a (24) and
//     sum b (24), one u64 of sum a^2 and sum b^2 (32 each) and one u32 of sum (a - b)^2: 20 bytes a class, 80 KiB at 4096 classes of
//     the 160 KiB a workgroup of gfx950 may declare, and three integer LDS atomics (two 64-bit, one 32-bit) for a run of pixels
//     instead of six. It clears only the classes of the launch's shift.
//   * THE FLUSH RULE. The squares grow by at most 255^2 a pixel, so a 32-bit field holds 66 051 pixels whatever they are; n's 16 bits
//     hold 65 535 and a 24-bit sum 65 793. A workgroup counts chunks of whole region rows of at most kLevelFlushPixels = 65 535 pixels each (level_geometry; a
//     row has at most 16 364) and keeps the number of pixels it has counted since its last flush, the same in every thread. Before a
//     chunk that would take that number past kLevelFlushPixels it flushes: every class whose n is not zero adds its non-zero words to
//     the query's u64 table with integer global atomics (the caller zeroes the tables on the stream) and is cleared; after its last
//     chunk it flushes once more. So no field ever exceeds its width (65 535 < 2^16, 65 535 x 255 < 2^24, 65 535 x 255^2 < 2^32:
//     asserted below) and nothing carries into its neighbour, also when every pixel falls into one class; a workgroup that counts a
//     single chunk scans its table once.
//   * Each region pixel is counted exactly once: chunks partition the rows, the threads of a workgroup partition a chunk's groups of
//     four pixels. All additions are integer and commute, so the tables are exact and identical from call to call in any order.
//   * A thread takes 4 consecutive pixels of a row (the last group of a row: the w % 4 that remain): 16 B of side a, 4 B of side b, 8 B
//     of the source, none naturally aligned (byte copies from pointers of known lesser alignment, as in k_joint), the loads of
//     kLevelQuads groups issued before the first is counted. Neighbouring pixels of one class are summed in registers first and added
//     as one run: a flat source, the most contended case, makes a quarter of the atomics.
//   * Chunks hold at least kLevelMinChunkPixels pixels where the region has them, so that clearing and scanning up to 4096 classes (4 a
//     thread) stays behind the counting (16 pixels, 12 atomics at the least, a thread).
//   * A launch has kLevelMaxBlocks = 128 workgroups, shared by its queries, not one for each of the 256 CUs: every workgroup adds up to
//     4096 x 6 words to the SAME global table, and those contended atomics, not the counting, bound the launch. MEASURED (DESIGN.md
//     section 4): 3072^2, 256 / 128 / 64 workgroups: 132 / 110 / 123 us.
// No float beyond out_u8's quantisation of side a, no f64, no order-dependent sum.
#include <algorithm>

#include "study_device.h"

namespace musica {

constexpr int kLutThreads = 1024;
constexpr int kLutChunks = 4;     // chunks a thread moves at a time
constexpr int kLutBlocks = 256;   // at most one workgroup a CU: 128 KiB of LDS each
static_assert(kLutEntries * sizeof(uint16_t) <= 160 * 1024 && kLutEntries % (8 * kLutThreads) == 0, "the table fits a workgroup's LDS and stages in whole 16-byte words a thread");

// kLutChunks chunks of V pixels from chunk c0 on, kLutThreads chunks apart
template <int V>
__device__ __forceinline__ void lut_load(const uint16_t* __restrict__ src, long long chunks, long long c0, PixelChunk<V> (&v)[kLutChunks]) {
    typedef typename PixelWord<V>::type __attribute__((may_alias)) Word;
#pragma unroll
    for (int k = 0; k < kLutChunks; k++) {
        const long long c = c0 + k * kLutThreads;
        if (c < chunks) v[k].w = *reinterpret_cast<const Word*>(src + c * V);
    }
}
template <int V>
__device__ __forceinline__ void lut_store(uint16_t* __restrict__ out, long long chunks, long long c0, PixelChunk<V> (&v)[kLutChunks], const uint16_t* tab) {
    typedef typename PixelWord<V>::type __attribute__((may_alias)) Word;
#pragma unroll
    for (int k = 0; k < kLutChunks; k++) {
        const long long c = c0 + k * kLutThreads;
        if (c >= chunks) break;
#pragma unroll
        for (int i = 0; i < V; i++) v[k].px[i] = tab[v[k].px[i]];
        *reinterpret_cast<Word*>(out + c * V) = v[k].w;
    }
}

// chunks: n^2 / V; both planes aligned to 2 V bytes, lut (a device allocation of its own) to 16
template <int V>
__global__ __launch_bounds__(kLutThreads) void k_alter_lut(const uint16_t* __restrict__ src, uint16_t* __restrict__ out, long long chunks,
                                                           const uint16_t* __restrict__ lut) {
    __shared__ uint16_t tab[kLutEntries];
    const long long per_block = kLutThreads * kLutChunks;
    long long c0 = blockIdx.x * per_block + threadIdx.x;
    PixelChunk<V> v[kLutChunks];
    lut_load<V>(src, chunks, c0, v);   // in flight under the staging
    for (int i = threadIdx.x; i < kLutEntries / 8; i += kLutThreads) reinterpret_cast<uint4*>(tab)[i] = reinterpret_cast<const uint4*>(lut)[i];
    __syncthreads();
    while (c0 < chunks) {   // a chunk group starts inside the plane or lies outside it entirely
        lut_store<V>(out, chunks, c0, v, tab);
        c0 += gridDim.x * per_block;
        lut_load<V>(src, chunks, c0, v);
    }
}

void launch_alter_lut(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const uint16_t* d_lut) {
    const long long total = (long long)n * n;   // at most 2^28
    launch_by_width(
        [&](auto v) {
            constexpr int V = decltype(v)::value;
            const long long chunks = total / V, per_block = kLutThreads * kLutChunks;
            hipLaunchKernelGGL((k_alter_lut<V>), dim3((unsigned)std::min<long long>(kLutBlocks, (chunks + per_block - 1) / per_block)), dim3(kLutThreads), 0, st, src,
                               out, chunks, d_lut);
        },
        (int)total, src, out);
}

// ---- the levels ------------------------------------------------------------------------------------------------------------------------
constexpr int kLevelThreads = 1024;
constexpr int kLevelFlushPixels = 65535;        // the most a workgroup counts between two flushes
constexpr int kLevelMinChunkPixels = 16384;     // a chunk's pixels where the region has them
constexpr int kLevelQuads = 2;                  // 4-pixel groups a thread loads before it counts them
constexpr int kLevelMaxBlocks = 128;            // workgroups per launch, shared by its queries; a workgroup strides over the chunks beyond that
static_assert(kLevelFlushPixels < (1 << 16) && kLevelFlushPixels * 255ull < (1ull << 24) && kLevelFlushPixels * 255ull * 255ull < (1ull << 32),
              "THE FLUSH RULE: what a workgroup counts between two flushes fits n's 16 bits, a sum's 24 and a sum of squares' 32, every pixel in one class");
static_assert(16384 <= kLevelFlushPixels, "a chunk of one row (N <= 16384) is within the rule");
static_assert(kLevelMaxClasses == (65535 >> kLevelMinShift) + 1 && kLevelMaxClasses * (2 * sizeof(unsigned long long) + sizeof(uint32_t)) <= 160 * 1024,
              "a u16 source >> shift, shift >= kLevelMinShift, indexes the LDS table, and the table fits a workgroup's LDS");
static_assert(kLevelMaxBlocks / kLevelMaxQueries >= 1, "every query of a launch gets a workgroup");

typedef __attribute__((address_space(1))) uint16_t GlobalU16;

// the classes of n >= 1 consecutive source pixels at p (2-byte aligned): the first four when n >= 4 (one 8-byte load)
__device__ __forceinline__ void load_classes4(const GlobalU16* p, int n, int shift, uint32_t (&k)[4]) {
    if (n >= 4) {
        uint16_t v[4];
        __builtin_memcpy(v, p, 8);
#pragma unroll
        for (int i = 0; i < 4; i++) k[i] = (uint32_t)v[i] >> shift;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) k[i] = i < n ? (uint32_t)p[i] >> shift : 0u;
}

// A query's table in LDS, packed (THE FLUSH RULE keeps every field within its bits)
struct LevelTable {
    unsigned long long sums[kLevelMaxClasses];      // n | sum a << 16 | sum b << 40
    unsigned long long squares[kLevelMaxClasses];   // sum a^2 | sum b^2 << 32
    uint32_t dd[kLevelMaxClasses];                  // sum (a - b)^2
};

// A run of neighbouring pixels of one class, summed in registers (at most 4 pixels: every word below 2^19)
struct LevelRun {
    uint32_t k, n, a, b, dd, aa, bb;
};
__device__ __forceinline__ void level_emit(LevelTable& tab, const LevelRun& r) {
    atomicAdd(&tab.sums[r.k], (unsigned long long)r.n | ((unsigned long long)r.a << 16) | ((unsigned long long)r.b << 40));
    atomicAdd(&tab.squares[r.k], (unsigned long long)r.aa | ((unsigned long long)r.bb << 32));
    atomicAdd(&tab.dd[r.k], r.dd);
}

// npx (1 .. 4) pixels: a and b packed a byte each, their classes in k
__device__ __forceinline__ void level_count(LevelTable& tab, uint32_t wa, uint32_t wb, const uint32_t (&k)[4], int npx) {
    LevelRun r = {k[0], 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i >= npx) break;
        if (k[i] != r.k) {
            level_emit(tab, r);
            r = {k[i], 0u, 0u, 0u, 0u, 0u, 0u};
        }
        const uint32_t a = (wa >> (8 * i)) & 0xFFu, b = (wb >> (8 * i)) & 0xFFu;
        const uint32_t d = a > b ? a - b : b - a;
        r.n += 1u;
        r.a += a;
        r.b += b;
        r.dd += d * d;
        r.aa += a * a;
        r.bb += b * b;
    }
    level_emit(tab, r);
}

__device__ __forceinline__ void level_clear(LevelTable& tab, int classes) {
    for (int k = threadIdx.x; k < classes; k += kLevelThreads) {
        tab.sums[k] = 0ull;
        tab.squares[k] = 0ull;
        tab.dd[k] = 0u;
    }
}

// THE FLUSH RULE's flush: the classes that were touched (n is not zero), unpacked, into the query's u64 table, and cleared. The
// caller's barriers stand around it.
__device__ __forceinline__ void level_flush(LevelTable& tab, GlobalU64* out, int classes) {
    for (int k = threadIdx.x; k < classes; k += kLevelThreads) {
        const unsigned long long sums = tab.sums[k];
        if (sums == 0ull) continue;   // no pixel of the class since the last flush
        const unsigned long long squares = tab.squares[k];
        const unsigned long long v[kLevelWords] = {sums & 0xFFFFull, (sums >> 16) & 0xFFFFFFull, sums >> 40, tab.dd[k], squares & 0xFFFFFFFFull, squares >> 32};
#pragma unroll
        for (int j = 0; j < kLevelWords; j++)
            if (v[j]) atomicAdd((unsigned long long*)(out + (size_t)k * kLevelWords + j), v[j]);
        tab.sums[k] = 0ull;
        tab.squares[k] = 0ull;
        tab.dd[k] = 0u;
    }
}

__global__ __launch_bounds__(kLevelThreads) void k_sim_levels(const LevelQueryDev* __restrict__ qs, int shift, int classes, unsigned long long* __restrict__ tables) {
    __shared__ LevelTable tab;
    const LevelQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.chunks) return;   // whole workgroup: the grid is sized for the query with the most chunks
    const int t = threadIdx.x;
    GlobalU64* out = (GlobalU64*)tables + q.table;
    level_clear(tab, classes);
    __syncthreads();
    const int groups = (q.w + 3) >> 2;   // of a row, the last one ragged
    int pending = 0;                     // pixels counted since the last flush: the same in every thread
    for (int chunk = blockIdx.x; chunk < q.chunks; chunk += gridDim.x) {
        const int r0 = chunk * q.chunk_rows;
        const int rows = min(q.chunk_rows, q.h - r0);
        if (pending + rows * q.w > kLevelFlushPixels) {   // uniform over the workgroup
            __syncthreads();
            level_flush(tab, out, classes);
            __syncthreads();
            pending = 0;
        }
        pending += rows * q.w;
        const GlobalF32* __restrict__ pa = (const GlobalF32*)q.a + (size_t)r0 * q.a_pitch;
        const GlobalU8* __restrict__ pb = (const GlobalU8*)q.b + (size_t)r0 * q.b_pitch;
        const GlobalU16* __restrict__ ps = (const GlobalU16*)q.s + (size_t)r0 * q.s_pitch;
        const int items = rows * groups;
        for (int i0 = t; i0 < items; i0 += kLevelQuads * kLevelThreads) {
            uint32_t wa[kLevelQuads], wb[kLevelQuads], k[kLevelQuads][4];
            int npx[kLevelQuads];
#pragma unroll
            for (int u = 0; u < kLevelQuads; u++) {   // all loads of the groups first
                const int i = i0 + u * kLevelThreads;
                npx[u] = 0;
                if (i < items) {
                    const int r = i / groups, c = (i - r * groups) << 2;
                    npx[u] = min(4, q.w - c);
                    wa[u] = load_quant4(pa + (size_t)r * q.a_pitch + c, npx[u]);
                    wb[u] = load_bytes4(pb + (size_t)r * q.b_pitch + c, npx[u]);
                    load_classes4(ps + (size_t)r * q.s_pitch + c, npx[u], shift, k[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < kLevelQuads; u++)
                if (npx[u] > 0) level_count(tab, wa[u], wb[u], k[u], npx[u]);
        }
    }
    __syncthreads();
    level_flush(tab, out, classes);
}

void level_geometry(LevelQueryDev& q, int count) {
    const int blocks = kLevelMaxBlocks / count;
    const int most = kLevelFlushPixels / q.w, least = (kLevelMinChunkPixels + q.w - 1) / q.w;   // most >= 4: w <= 16364
    q.chunk_rows = std::max(1, std::min(most, std::max(least, (q.h + blocks - 1) / blocks)));
    q.chunks = (q.h + q.chunk_rows - 1) / q.chunk_rows;
}

void launch_sim_levels(hipStream_t st, const LevelQueryDev* d_qs, int count, int max_chunks, int shift, unsigned long long* tables) {
    hipLaunchKernelGGL(k_sim_levels, dim3((unsigned)std::min(max_chunks, kLevelMaxBlocks / count), 1, (unsigned)count), dim3(kLevelThreads), 0, st, d_qs, shift,
                       (65535 >> shift) + 1, tables);
}

}  // namespace musica
