// kernels_cooccurrence.hip — the texture metric of the study (musica_sim_cooccurrence, include/musica.h; metrics.cooccurrence_statistics):
// the gray-level co-occurrence matrices of a comparison. The level of an 8-bit pixel v is v >> (8 - log2 G), G in {8, 16, 32, 64}; per
// distance d (1 .. 16) and direction 0 (d, 0), 45 (d, d), 90 (0, d), 135 (-d, d) degrees a pair (p, p + offset) counts on a side where both
// pixels lie inside the region on that side, once, in T[level(p)][level(p + offset)]. Side a is the graded f32 plane of a batch image
// quantised with out_u8 while it is read (load_quant4: exactly what k_sim reads), side b a reference slot. No float arithmetic anywhere.
//
// k_cooccurrence<G>: a query owns blockIdx.z; blockIdx.y = 2 k + side is ONE distance and ONE side of it, which `groups` PERSISTENT
// workgroups of kStudyThreads threads share: workgroup g takes the 64 x 64 tiles g, g + groups, .. of the region (tile_geom). ONE side a
// workgroup: the four direction tables of a workgroup are 4 G^2 counters instead of 8 G^2, a window is one plane, and a pass still reads
// 4 + 1 bytes a pixel per distance, 4 in the workgroups of side a and 1 in those of side b.
//   stage    the tile and its halo, d columns on the left, d on the right and d rows below, clipped to the region, as packed LEVELS in
//            LDS (stage_halo_window: the bytes of a word shifted and masked at once): tile pixel (tx, ty) is byte 16 + tx of window row
//            ty, whatever d, so a thread's words are aligned. A pair belongs to the tile of its FIRST pixel; a halo pixel is only ever
//            a second pixel, and no pixel outside the region (or the plane) is read: the other bytes of the window are 0 and a pair
//            that would use one is not counted (the run bounds below).
//   count    thread t takes the 16 consecutive first pixels 16 q .. 16 q + 15 (q = t & 3) of tile row t / 4: one ds_read_b128; the
//            second pixels of 90 degrees are the aligned b128 d rows below, those of 0 and 45 the five words d bytes on in the row and
//            in the row d below, those of 135 the five words d bytes back, turned by v_alignbyte_b32 (shifted_words) so that byte k of
//            the second words is the partner of byte k of the first. Which k of a run count is two integers a direction: lo <= k < hi.
//   add      into the workgroup's u32 tables in LDS, kept over all its tiles (THE WIDTH RULE), see CONTENTION.
//   flush    once a workgroup, behind its last tile: the replicas of a counter are summed and every NON-ZERO counter goes to the
//            query's table, which the caller zeroes on the stream, with one u32 global atomic: one a touched counter, never one a pair.
// THE WIDTH RULE. The counters are u32, not packed u16: there is no flush rule because there is nothing to wrap. A region's side is at
// most 16364, so a table holds at most 16364^2 < 2^28 pairs; a workgroup's counter, a replica of it and the global word are each at most
// that. u32 at G = 64 costs 64 KiB of LDS a workgroup where packed u16 pairs would take 32: two workgroups a compute unit.
// CONTENTION. On a natural image nearly all pairs fall next to the diagonal, and the lanes of a wavefront (16 tile rows x 4 runs, one
// neighbourhood) ask for the same few counters at once; the LDS serialises equal addresses of one instruction. Two means, both measured
// (DESIGN.md section 4):
//   runs      a lane walks its 16 pairs of a direction in order and adds a run of equal (i, j) with ONE ds_add_u32 of the run's length:
//             on a flat area 1 atomic for 16 pairs, on noise 16 for 16 plus a compare and a branch a pair, which is its cost: at
//             3072^2 on a processed phantom 107 against 152 us at G = 32 and 123 against 216 at G = 64 without runs, but 106 against
//             86 at G = 8, and 15 - 25 % slower than without on random planes.
//   replicas  R copies of every counter, R = 16, 8, 2, 1 at G = 8, 16, 32, 64 (16, 32, 32, 64 KiB), the copy of lane t being t mod R and
//             the copies of a counter neighbouring words: R lanes that want one counter hit R different banks. Its cost is LDS (the
//             occupancy) and R reads a counter in the flush; at G = 64 there is no room for a second copy. 5 - 7 % faster than one
//             copy at one distance on the phantom, but SLOWER at four distances with G = 16 and 32 (253 against 221 us, 275 against 258).
// Against one global atomic a pair the shipped form is 600 - 1100 times faster on the phantom and 25 - 180 times on random planes.
// Integer sums commute: the tables are exact and byte-identical from call to call and for any number of workgroups
// (MUSICA_COOCCURRENCE_GROUPS, musica_study.hip).
// MUSICA_COOCCURRENCE_GLOBAL_ATOMICS (a devtools/build_variant.sh build, for the A/B of DESIGN.md section 4; not shipped) replaces the
// LDS tables with one global atomic per pair; MUSICA_COOCCURRENCE_NO_RUNS adds every pair on its own and MUSICA_COOCCURRENCE_ONE_COPY
// keeps one copy of a counter (likewise).
#include "study_device.h"

namespace musica {

constexpr int kCoocPad = kCooccurrenceMaxDistance;                    // window bytes left of the tile's first column
constexpr int kCoocWinRows = kSimTile + kCooccurrenceMaxDistance;     // 80
constexpr int kCoocWords = (kCoocPad + kSimTile + kCooccurrenceMaxDistance) / 4 + 1;   // 25 staged words a row: the fifth word of the last run at d = 16
constexpr int kCoocPitch = 28;                                        // words between the window's rows: a multiple of 4 for ds_read_b128
static_assert(kSimTile == 64 && kStudyThreads == 256, "a thread takes 16 first pixels of a row: four lanes a row, 64 rows");
static_assert(kCoocPad % 4 == 0 && kCoocPad >= kCooccurrenceMaxDistance && kCoocPitch % 4 == 0 && kCoocPitch >= kCoocWords, "aligned runs; the words d bytes back exist");

constexpr int cooccurrence_replicas(int G) {
#ifdef MUSICA_COOCCURRENCE_ONE_COPY
    return 1;
#else
    return G == 8 ? 16 : G == 16 ? 8 : G == 32 ? 2 : 1;
#endif
}

// The pairs lo <= k < hi of a run: first pixel byte k of F, second byte k of S (levels), into the direction's table.
template <int G, int R>
__device__ __forceinline__ void cooccurrence_run(uint32_t* __restrict__ tab, GlobalU32* __restrict__ out, const uint32_t (&F)[4], const uint32_t (&S)[4], int lo, int hi,
                                                 int copy) {
    uint32_t cur = 0u, n = 0u;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t bin = ((F[k >> 2] >> (8 * (k & 3))) & 0xFFu) * G + ((S[k >> 2] >> (8 * (k & 3))) & 0xFFu);
        if (k < lo || k >= hi) continue;
#if defined(MUSICA_COOCCURRENCE_GLOBAL_ATOMICS)
        atomicAdd((uint32_t*)(out + bin), 1u);
#elif defined(MUSICA_COOCCURRENCE_NO_RUNS)
        atomicAdd(&tab[bin * R + copy], 1u);
#else
        if (n && bin != cur) {
            atomicAdd(&tab[cur * R + copy], n);
            n = 0u;
        }
        cur = bin;
        n++;
#endif
    }
    if (n) atomicAdd(&tab[cur * R + copy], n);
}

// The five words at p turned by sh bytes: byte k of v is byte k + sh of the 20 bytes at p
__device__ __forceinline__ void cooccurrence_turned(const uint32_t* p, uint32_t sh, uint32_t (&v)[4]) { shifted_words(p[0], p[1], p[2], p[3], p[4], sh, v); }
__device__ __forceinline__ void cooccurrence_aligned(const uint32_t* p, uint32_t (&v)[4]) {
    const uint4 w = *reinterpret_cast<const uint4*>(p);
    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
}

template <int G>
__global__ __launch_bounds__(kStudyThreads) void k_cooccurrence(const CooccurrenceQueryDev* __restrict__ qs, CooccurrenceDistances dist, uint32_t* __restrict__ tables) {
    constexpr int R = cooccurrence_replicas(G), BINS = G * G;
    constexpr int SHIFT = G == 8 ? 5 : G == 16 ? 4 : G == 32 ? 3 : 2;
    constexpr uint32_t MASK = 0x01010101u * (uint32_t)(G - 1);
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "levels");
    __shared__ __attribute__((aligned(16))) uint32_t win[kCoocWinRows * kCoocPitch];
#ifdef MUSICA_COOCCURRENCE_GLOBAL_ATOMICS
    uint32_t* const tab = nullptr;
#else
    __shared__ uint32_t tab[4 * BINS * R];
#endif
    const CooccurrenceQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.groups) return;   // whole workgroup: the grid is sized for the query with the most groups
    const int t = threadIdx.x, row = t >> 2, c0 = 16 * (t & 3), copy = t & (R - 1);
    const int slice = (int)blockIdx.y >> 1, side = (int)blockIdx.y & 1, d = dist.d[slice];   // blockIdx.y < 2 dist.count; 1 <= d <= 16
    // table [slice][direction][side]: direction dir is 2 BINS words further
    GlobalU32* const out = (GlobalU32*)tables + q.table + (size_t)(slice * 8 + side) * BINS;
#ifndef MUSICA_COOCCURRENCE_GLOBAL_ATOMICS
    for (int i = t; i < 4 * BINS * R; i += kStudyThreads) tab[i] = 0u;
#endif
    const uint32_t* const first = win + row * kCoocPitch + (kCoocPad + c0) / 4;   // the run's first pixels; word >= 4
    const uint32_t* const below = first + d * kCoocPitch;                         // row + d <= 79
    const int on = d >> 2, back = (d + 3) >> 2;                                    // back <= 4: never before the row's first word
    const uint32_t on_sh = (uint32_t)d & 3u, back_sh = (4u - on_sh) & 3u;
    const auto levels = [](uint32_t w) { return (w >> SHIFT) & MASK; };

    const int tiles = q.tiles_x * q.tiles_y;
    for (int tile = blockIdx.x; tile < tiles; tile += q.groups) {
        const TileGeom g = tile_geom(tile, q.tiles_x, q.w, q.h);
        __syncthreads();   // the last tile's window is read; the first time: the tables are cleared
        const int x_lo = max(g.x0 - d, 0), x_hi = min(g.x0 + g.tw + d, q.w), y_hi = min(g.y0 + g.th + d, q.h);
        if (side) stage_halo_window((const GlobalU8*)q.b, q.b_pitch, g.x0 - kCoocPad, g.y0, x_lo, x_hi, g.y0, y_hi, win, kCoocPitch, kCoocWords, kSimTile + d, levels);
        else stage_halo_window((const GlobalF32*)q.a, q.a_pitch, g.x0 - kCoocPad, g.y0, x_lo, x_hi, g.y0, y_hi, win, kCoocPitch, kCoocWords, kSimTile + d, levels);
        __syncthreads();
        if (row < g.th) {   // the tile's rows; a ragged last tile has fewer
            const int in_tile = g.tw - c0;                          // the first pixel k of the run lies in the tile: k < in_tile
            const int right = min(in_tile, q.w - g.x0 - d - c0);    // its partner d columns on lies in the region: k < right
            const int left = d - g.x0 - c0;                         // its partner d columns back lies in the region: k >= left
            uint32_t F[4], S[4];
            cooccurrence_aligned(first, F);
            cooccurrence_turned(first + on, on_sh, S);
            cooccurrence_run<G, R>(tab, out, F, S, 0, right, copy);
            if (g.y0 + row + d < q.h) {
                cooccurrence_turned(below + on, on_sh, S);
                cooccurrence_run<G, R>(tab + BINS * R, out + 2 * BINS, F, S, 0, right, copy);
                cooccurrence_aligned(below, S);
                cooccurrence_run<G, R>(tab + 2 * BINS * R, out + 4 * BINS, F, S, 0, in_tile, copy);
                cooccurrence_turned(below - back, back_sh, S);
                cooccurrence_run<G, R>(tab + 3 * BINS * R, out + 6 * BINS, F, S, left, in_tile, copy);
            }
        }
    }
#ifndef MUSICA_COOCCURRENCE_GLOBAL_ATOMICS
    __syncthreads();
    for (int i = t; i < 4 * BINS; i += kStudyThreads) {
        uint32_t sum = 0u;
#pragma unroll
        for (int r = 0; r < R; r++) sum += tab[i * R + r];
        const int dir = i / BINS, bin = i - dir * BINS;
        if (sum) atomicAdd((uint32_t*)(out + dir * 2 * BINS + bin), sum);   // inside the query's [slice] tables: (slice * 8 + side + 2 dir) * BINS + bin
    }
#endif
}

template <int G>
static void launch_cooccurrence(hipStream_t st, const CooccurrenceQueryDev* d_qs, int count, int max_groups, const CooccurrenceDistances& dist, uint32_t* tables) {
    hipLaunchKernelGGL(k_cooccurrence<G>, dim3((unsigned)max_groups, 2u * (unsigned)dist.count, (unsigned)count), dim3(kStudyThreads), 0, st, d_qs, dist, tables);
}

void launch_sim_cooccurrence(hipStream_t st, const CooccurrenceQueryDev* d_qs, int count, int max_groups, int levels, const CooccurrenceDistances& dist, uint32_t* tables) {
    switch (levels) {
        case 8: launch_cooccurrence<8>(st, d_qs, count, max_groups, dist, tables); break;
        case 16: launch_cooccurrence<16>(st, d_qs, count, max_groups, dist, tables); break;
        case 32: launch_cooccurrence<32>(st, d_qs, count, max_groups, dist, tables); break;
        case 64: launch_cooccurrence<64>(st, d_qs, count, max_groups, dist, tables); break;
        default: return;
    }
}

}  // namespace musica
