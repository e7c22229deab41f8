// kernels_lattice.hip — the lattice sums of the study (musica_sim_lattice, include/musica.h; metrics.lattice_statistics): a comparison's
// sums folded by the position modulo a period P in {2, 4, 8, 16, 32}. Over the pixels (i, j) of a query with i < w - 1 and j < h - 1 (every
// counted pixel has a right and a lower neighbour inside the region), the class of a pixel is [(ay + j + o) mod P][(ax + i + o) mod P];
// per class the eight exact sums n, a, b, (a - b)^2, the squared horizontal step of a and of b, the squared vertical step of a and of b.
// Side a is the graded f32 plane of a batch image quantised with out_u8 while it is read (load_quant4: exactly what k_sim and k_order
// read), side b a reference slot. No float anywhere.
//
// k_lattice<P>: a query owns blockIdx.z and `groups` PERSISTENT workgroups of kStudyThreads threads; workgroup g takes the 64 x 64
// tiles g, g + groups, .. of the query's (w - 1) x (h - 1) counted pixels (tile_geom), at most kLatticeGroupTiles of them.
//   stage    the (tw + 1) x (th + 1) windows of both sides, at most 65 x 65, once, as packed bytes in LDS (stage_windows): 17 words a
//            row, zeros beyond a ragged tile, nothing outside the region is read: 4 + 1 bytes a pixel from memory, once.
//   sums     lane l of every wavefront owns COLUMN l of the tile and wavefront v the rows v, v + 4, .. . Tiles start at multiples of
//            64 and 64 is a multiple of P, so a lane's column phase is one value for the whole launch, and the row phase of the row
//            v + 4k is one of NP = max(P / 4, 1) values, chosen by k mod NP: a compile-time register index. A thread therefore keeps
//            NP x 8 u32 sums in REGISTERS over all its tiles (64 registers at P = 32) and touches neither LDS nor memory per pixel.
//   combine  once a workgroup, behind its last tile: for P <= 8 the lanes of equal column phase inside a row of 16 lanes are summed by
//            DPP adds (row_shr:P, 2P .. 8: wave_isum's steps from P on), which leaves the sums in the last P lanes of the row; those
//            lanes (every lane for P >= 16) add into the workgroup's u32 table in LDS, 8 P^2 words, at most 32 KiB, laid out
//            [field][row phase][column phase] so that the lanes of an add lie on neighbouring banks. The four rows of a wavefront
//            (two lanes at P = 32) meet on an address: LDS atomics, NP x 8 a wavefront and launch.
//   flush    the workgroup stores its 8 P^2 words, zeros included, as its own partial table: plain coalesced stores, no atomics.
// k_lattice_fold: a thread takes a table word and one of 16 slices of the query's partial tables, sums them in u64 (coalesced reads: the
// threads of a wavefront take neighbouring words of one partial table) and adds the sum to the query's u64 table, which the caller
// zeroes on the stream, with one 64-bit integer global atomic: 16 adds a word. Integer sums commute: exact and byte-identical from call
// to call. The first form flushed with 64-bit global atomics instead: at P = 8 all workgroups of a launch met on 32 cache lines, and the
// flush, not the pixels, set the time (DESIGN.md section 4 has both measurements).
// THE 32-BIT RULE. The largest addend is (a - b)^2 <= 65025 a pixel. A workgroup counts at most kLatticeGroupTiles tiles of 4096
// pixels, of which a class holds at most 4096 / P^2 <= 1024 each: 64 x 1024 = 65536 pixels a class and workgroup, below the 66051 at
// which 65025 n reaches 2^32 (asserted below). The host sizes `groups` accordingly (launchers.h: lattice_groups). The fold widens to 64 bits.
#include "study_device.h"

namespace musica {

constexpr int kLatticeWinWords = (kSimTile + 1 + 3) / 4;   // words of a staged window row: 65 pixels
constexpr int kLatticeWinRows = kSimTile + 1;
constexpr int kLatticeTrips = kSimTile / kStudyWaves;      // rows of a tile that a wavefront takes
static_assert(kLatticeWinWords == 17 && kLatticeWinRows == 65 && kLatticeTrips == 16 && kSimTile == 64, "a lane a column, 16 rows a wavefront");
static_assert((unsigned long long)kLatticeGroupTiles * (kSimTile * kSimTile / 4) * 65025ull < (1ull << 32),
              "THE 32-BIT RULE: a class's sum of (a - b)^2 over a workgroup's tiles at P = 2");
static_assert(kLatticeWords == 8, "n, a, b, dd and the four squared steps");

__device__ __forceinline__ int lattice_byte(const uint32_t* __restrict__ win, int row, int x) {
    return (int)((win[row * kLatticeWinWords + (x >> 2)] >> (8 * (x & 3))) & 0xFFu);
}

template <int CTRL>
__device__ __forceinline__ void lattice_shr_add(uint32_t& v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);   // a lane without a source adds 0
}

template <int P>
__global__ __launch_bounds__(kStudyThreads) void k_lattice(const LatticeQueryDev* __restrict__ qs, uint32_t* __restrict__ part) {
    constexpr int NP = P >= 4 ? P / 4 : 1;     // row phases of a wavefront
    constexpr int CLASSES = P * P;
    __shared__ uint32_t wa[kLatticeWinRows * kLatticeWinWords], wb[kLatticeWinRows * kLatticeWinWords];
    __shared__ uint32_t lat[kLatticeWords * CLASSES];
    const LatticeQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.groups) return;   // whole workgroup: the grid is sized for the query with the most groups
    const int t = threadIdx.x, l = t & 63, wave = t >> 6;
    for (int i = t; i < kLatticeWords * CLASSES; i += kStudyThreads) lat[i] = 0u;

    uint32_t acc[NP][kLatticeWords];
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int f = 0; f < kLatticeWords; f++) acc[p][f] = 0u;

    const int tiles = q.tiles_x * q.tiles_y;
    for (int tile = blockIdx.x; tile < tiles; tile += q.groups) {
        const TileGeom g = tile_geom(tile, q.tiles_x, q.w - 1, q.h - 1);   // of the counted pixels: window pixel (0, 0) is region pixel (x0, y0)
        __syncthreads();   // the last tile's windows are read
        stage_windows((const GlobalF32*)q.a + (ptrdiff_t)g.y0 * q.a_pitch + g.x0, q.a_pitch, (const GlobalU8*)q.b + (ptrdiff_t)g.y0 * q.b_pitch + g.x0, q.b_pitch,
                      g.tw + 1, g.th + 1, wa, wb, kLatticeWinWords, kLatticeWinWords, kLatticeWinRows);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kLatticeTrips; k++) {
            const int r = wave + kStudyWaves * k;   // rows r, r + 1 <= 64 and columns l, l + 1 <= 64: inside the staged window
            if (r >= g.th || l >= g.tw) continue;
            const int a0 = lattice_byte(wa, r, l), a1 = lattice_byte(wa, r, l + 1), a2 = lattice_byte(wa, r + 1, l);
            const int b0 = lattice_byte(wb, r, l), b1 = lattice_byte(wb, r, l + 1), b2 = lattice_byte(wb, r + 1, l);
            uint32_t(&s)[kLatticeWords] = acc[k % NP];
            s[0] += 1u;
            s[1] += (uint32_t)a0;
            s[2] += (uint32_t)b0;
            s[3] += (uint32_t)((a0 - b0) * (a0 - b0));
            s[4] += (uint32_t)((a1 - a0) * (a1 - a0));
            s[5] += (uint32_t)((b1 - b0) * (b1 - b0));
            s[6] += (uint32_t)((a2 - a0) * (a2 - a0));
            s[7] += (uint32_t)((b2 - b0) * (b2 - b0));
        }
    }
    __syncthreads();   // lat is zeroed; every lane is back

    // the lanes of equal column phase inside a row of 16 lanes: all 64 lanes are active here
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int f = 0; f < kLatticeWords; f++) {
            if (P <= 2) lattice_shr_add<0x112>(acc[p][f]);   // row_shr:2
            if (P <= 4) lattice_shr_add<0x114>(acc[p][f]);   // row_shr:4
            if (P <= 8) lattice_shr_add<0x118>(acc[p][f]);   // row_shr:8
        }
    const int cp = (q.phase_x + l) & (P - 1);
    if (P >= 16 || (l & 15) >= 16 - P) {
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int rp = (q.phase_y + wave + kStudyWaves * p) & (P - 1);
#pragma unroll
            for (int f = 0; f < kLatticeWords; f++)
                if (acc[p][f]) atomicAdd(&lat[f * CLASSES + rp * P + cp], acc[p][f]);
        }
    }
    __syncthreads();
    GlobalU32* mine = (GlobalU32*)part + q.part + (size_t)blockIdx.x * (kLatticeWords * CLASSES);   // blockIdx.x < q.groups: inside the query's partials
    for (int i = t; i < kLatticeWords * CLASSES; i += kStudyThreads) mine[i] = lat[i];
}

// Word i = field * P^2 + class of the partial tables slice, slice + kLatticeFoldSlices, .. of a query (blockIdx.y: the slice), summed
// and added to word class * 8 + field of its table. Eight loads in flight a thread: one after the other, 2304 partial tables took 541 us.
constexpr int kLatticeFoldSlices = 16;
__global__ __launch_bounds__(kStudyThreads) void k_lattice_fold(const LatticeQueryDev* __restrict__ qs, const uint32_t* __restrict__ part, int classes,
                                                                 unsigned long long* __restrict__ tables) {
    const LatticeQueryDev q = qs[blockIdx.z];
    const int i = (int)(blockIdx.x * kStudyThreads + threadIdx.x), words = kLatticeWords * classes;
    if (i >= words) return;
    const GlobalU32* p = (const GlobalU32*)part + q.part + i;
    unsigned long long sum = 0ull;
    int g = (int)blockIdx.y;
    for (; g + 7 * kLatticeFoldSlices < q.groups; g += 8 * kLatticeFoldSlices) {
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = p[(size_t)(g + k * kLatticeFoldSlices) * words];
#pragma unroll
        for (int k = 0; k < 8; k++) sum += v[k];
    }
    for (; g < q.groups; g += kLatticeFoldSlices) sum += p[(size_t)g * words];
    const int f = i / classes, c = i - f * classes;
    if (sum) atomicAdd((unsigned long long*)((GlobalU64*)tables + q.table + (size_t)c * kLatticeWords + f), sum);
}

void launch_sim_lattice(hipStream_t st, const LatticeQueryDev* d_qs, int count, int max_groups, int period, uint32_t* part, unsigned long long* tables) {
    const dim3 grid((unsigned)max_groups, 1, (unsigned)count), block(kStudyThreads);
    switch (period) {
        case 2: hipLaunchKernelGGL(k_lattice<2>, grid, block, 0, st, d_qs, part); break;
        case 4: hipLaunchKernelGGL(k_lattice<4>, grid, block, 0, st, d_qs, part); break;
        case 8: hipLaunchKernelGGL(k_lattice<8>, grid, block, 0, st, d_qs, part); break;
        case 16: hipLaunchKernelGGL(k_lattice<16>, grid, block, 0, st, d_qs, part); break;
        case 32: hipLaunchKernelGGL(k_lattice<32>, grid, block, 0, st, d_qs, part); break;
        default: return;
    }
    const int words = kLatticeWords * period * period;
    hipLaunchKernelGGL(k_lattice_fold, dim3((unsigned)((words + kStudyThreads - 1) / kStudyThreads), kLatticeFoldSlices, (unsigned)count), block, 0, st, d_qs, part,
                       period * period, tables);
}

}  // namespace musica
