// kernels_displace.hip — exact block matching of the study (musica_sim_displace, include/musica.h; harness.py displacement_table): the
// sum of squared differences between a region of a batch image's 8-bit output (side a: the graded f32 plane quantised with out_u8 while
// it is read, exactly what k_sim compares) and the same region of a reference slot (side b) displaced by every integer shift
// (dx, dy) in [-R, R]^2, per 64 x 64 tile of the region and, folded, for the whole region. S = 2 R + 1.
//
// k_displace: one workgroup of 256 threads per tile, the query in blockIdx.z as in k_sim.
//   * Staging (the layout, the work items and the bank argument: study_device.h, packed byte windows). The tile of a goes into LDS
//     quantised once; pixels outside the region (a ragged last tile) are 0. The window of b the tile's candidates reach,
//     (tile_w + 2 R) x (tile_h + 2 R) bytes from (64 tx - R, 64 ty - R) of the region, goes into LDS from byte 0 of each row, whatever the
//     alignment of bx in the plane: the staging copy absorbs it (a word of 4 bytes from a pointer of alignment 1 is one global_load_dword
//     in gfx950's unaligned access mode). Bytes past the window are 0 and never loaded: musica_sim_displace refuses a query whose grown b
//     window leaves the plane, so everything that is loaded lies inside it.
//   * SSD = sum a^2 + sum b'^2 - 2 sum a b'. sum a^2 does not depend on the candidate and is taken once while a is staged. There are
//     S^2 * ceil(tile_h / 8) work items. Per 16 pixels of a row an item forms the four shifted words of b' and does eight
//     v_dot4_u32_u8: four for a b', four for b'^2. That is 2 multiply-adds per pixel and candidate, 0.5 dot4 instructions.
//   * Padding. Rows past tile_h are not visited. In the last, partial, 16 pixels of a ragged row b' is masked by the pixel's position in
//     the REGION (bytes at x >= tile_w are cleared after the shift), not by where its source byte lies: a padded pixel adds 0 to
//     sum a^2, sum a b' and sum b'^2 of every candidate, while a pixel inside the region sees b beyond the region's edge.
//   * An item adds sum b'^2 - 2 sum a b' (mod 2^32) to its candidate's entry of an LDS table with one integer LDS atomic; the entry plus
//     sum a^2 is the tile's SSD, at most 64 * 64 * 255^2 < 2^32, so the arithmetic mod 2^32 is exact. The tile table is written as u32.
//   * The tile's own argmin (smallest value, then smallest dx^2 + dy^2, then smallest dy, then smallest dx: the minimum of the 64-bit
//     key value << 32 | d^2 << 12 | (dy + R) << 6 | (dx + R)) is reduced over the workgroup; a tile whose argmin is not (0, 0) adds 1 to
//     the query's tiles_off with one integer atomic.
// k_displace_fold: the query's tile tables summed into its u64 table, a thread per candidate over a chunk of tiles, one 64-bit integer
// atomic per (candidate, chunk). Everything is integer arithmetic: exact, and the same from call to call whatever the order.
#include <algorithm>

#include "study_device.h"

namespace musica {

constexpr int kDispThreads = kStudyThreads;
constexpr int kDispMaxS = 2 * kSimMaxRadius + 1;
constexpr int kDispFoldChunks = 32;          // tile chunks of k_displace_fold

// 16 pixels of one row for one candidate: av the words of a, lo the word of b before b1 .. b4, sh the byte shift. `valid`: pixels of the
// 16 that lie in the region (MASK only).
template <bool MASK>
__device__ __forceinline__ void disp_chunk(const uint4 av, uint32_t lo, uint32_t b1, uint32_t b2, uint32_t b3, uint32_t b4, uint32_t sh,
                                           int valid, uint32_t& sab, uint32_t& sbb) {
    uint32_t v[4];
    shifted_words(lo, b1, b2, b3, b4, sh, v);
    const uint32_t a[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (MASK) {
            const int n = valid - 4 * k;   // uniform over the workgroup
            v[k] = n >= 4 ? v[k] : n <= 0 ? 0u : v[k] & ((1u << (8 * n)) - 1u);
        }
        sab = dot4(a[k], v[k], sab);
        sbb = dot4(v[k], v[k], sbb);
    }
}

__global__ __launch_bounds__(kDispThreads) void k_displace(const DisplaceQueryDev* __restrict__ qs, int radius, uint32_t* __restrict__ tile_tables,
                                                           uint32_t* __restrict__ tiles_off) {
    __shared__ __attribute__((aligned(16))) uint32_t sa[kSimTile * kByteTilePitch];
    __shared__ uint32_t sb[(kSimTile + 2 * kSimMaxRadius) * kByteWinPitch];
    __shared__ uint32_t tab[kDispMaxS * kDispMaxS];
    __shared__ uint32_t saa;
    __shared__ WaveSlots<unsigned long long> best;
    const DisplaceQueryDev q = qs[blockIdx.z];
    const int tile = blockIdx.x;
    if (tile >= q.tiles_x * q.tiles_y) return;   // whole workgroup: the grid is sized for the query with the most tiles
    const int t = threadIdx.x;
    const auto [x0, y0, tw, th] = tile_geom(tile, q.tiles_x, q.w, q.h);
    const int S = 2 * radius + 1, S2 = S * S;
    for (int i = t; i < S2; i += kDispThreads) tab[i] = 0u;
    if (t == 0) saa = 0u;
    __syncthreads();

    const GlobalF32* __restrict__ pa = (const GlobalF32*)q.a + (ptrdiff_t)y0 * q.a_pitch + x0;
    uint32_t aa = 0u;
    for (int i = t; i < kSimTile * 16; i += kDispThreads) {
        const int r = i >> 4, x = (i & 15) << 2;
        const uint32_t word = r < th && x < tw ? load_quant4(pa + (ptrdiff_t)r * q.a_pitch + x, tw - x) : 0u;
        sa[r * kByteTilePitch + (i & 15)] = word;
        aa = dot4(word, word, aa);
    }
    wave_sum(aa);
    if (wave_leader()) atomicAdd(&saa, aa);

    const int bw = tw + 2 * radius, bh = th + 2 * radius;   // the window of b in bytes and rows: inside the plane (the call's refusals)
    const GlobalU8* __restrict__ pb = (const GlobalU8*)q.b + (ptrdiff_t)(y0 - radius) * q.b_pitch + (x0 - radius);
    for (int i = t; i < bh * kByteWinWords; i += kDispThreads) {
        const int r = i / kByteWinWords, wd = i - r * kByteWinWords, j = wd << 2;
        uint32_t word = 0u;
        if (j < bw) {
            const GlobalU8* p = pb + (ptrdiff_t)r * q.b_pitch + j;
            if (j + 4 <= bw) {
                __builtin_memcpy(&word, p, 4);   // 1-byte aligned
            } else {
                for (int k = 0; k < bw - j; k++) word |= (uint32_t)p[k] << (8 * k);
            }
        }
        sb[r * kByteWinPitch + wd] = word;
    }
    __syncthreads();

    const int blocks = (th + kByteRows - 1) / kByteRows;
    const int full = tw >> 4, rest = tw & 15;
    for (int i = t; i < S2 * blocks; i += kDispThreads) {
        const int p = i / S2, c = i - p * S2;
        const int dyi = c / S, dxi = c - dyi * S;   // dy + R, dx + R
        const uint32_t sh = (uint32_t)(dxi & 3);
        const int y1 = min(th, (p + 1) * kByteRows);
        uint32_t sab = 0u, sbb = 0u;   // <= 8 * 64 * 255^2 < 2^25
        for (int y = p * kByteRows; y < y1; y++) {
            const uint4* ar = reinterpret_cast<const uint4*>(sa + y * kByteTilePitch);
            const uint32_t* br = sb + (y + dyi) * kByteWinPitch + (dxi >> 2);
            uint32_t lo = br[0];
            for (int ch = 0; ch < full; ch++) {
                const uint32_t b1 = br[4 * ch + 1], b2 = br[4 * ch + 2], b3 = br[4 * ch + 3], b4 = br[4 * ch + 4];
                disp_chunk<false>(ar[ch], lo, b1, b2, b3, b4, sh, 16, sab, sbb);
                lo = b4;
            }
            if (rest) {   // full <= 3: words up to (dxi >> 2) + 16 <= 24 < kByteWinWords
                const uint32_t b1 = br[4 * full + 1], b2 = br[4 * full + 2], b3 = br[4 * full + 3], b4 = br[4 * full + 4];
                disp_chunk<true>(ar[full], lo, b1, b2, b3, b4, sh, rest, sab, sbb);
            }
        }
        atomicAdd(&tab[c], sbb - 2u * sab);
    }
    __syncthreads();

    uint32_t* __restrict__ out = tile_tables + q.tile_base + (size_t)tile * S2;
    unsigned long long key = ~0ull;
    for (int c = t; c < S2; c += kDispThreads) {
        const uint32_t v = tab[c] + saa;
        out[c] = v;
        const int dyi = c / S, dxi = c - dyi * S;
        const int dy = dyi - radius, dx = dxi - radius;
        const unsigned long long k = ((unsigned long long)v << 32) | ((unsigned long long)(dx * dx + dy * dy) << 12) | (unsigned long long)((dyi << 6) | dxi);
        key = k < key ? k : key;
    }
    key = wave_min(key);
    if (wave_leader()) best.put(key);
    __syncthreads();
    if (t == 0 && (uint32_t)(best.min() & 0xFFFu) != (uint32_t)((radius << 6) | radius)) atomicAdd(&tiles_off[blockIdx.z], 1u);
}

__global__ __launch_bounds__(kDispThreads) void k_displace_fold(const DisplaceQueryDev* __restrict__ qs, int S2, const uint32_t* __restrict__ tile_tables,
                                                                unsigned long long* __restrict__ tables) {
    const DisplaceQueryDev q = qs[blockIdx.z];
    const int c = blockIdx.x * kDispThreads + threadIdx.x;
    if (c >= S2) return;
    const int tiles = q.tiles_x * q.tiles_y;
    const int per = (tiles + (int)gridDim.y - 1) / (int)gridDim.y;
    const int t0 = blockIdx.y * per, t1 = min(tiles, t0 + per);
    const uint32_t* __restrict__ src = tile_tables + q.tile_base + c;
    unsigned long long sum = 0ull;
    for (int i = t0; i < t1; i++) sum += src[(size_t)i * S2];
    if (sum) atomicAdd(&tables[(size_t)blockIdx.z * S2 + c], sum);
}

void launch_displace(hipStream_t st, const DisplaceQueryDev* d_qs, int count, int max_tiles, int radius, uint32_t* tile_tables,
                     unsigned long long* tables, uint32_t* tiles_off) {
    const int S2 = (2 * radius + 1) * (2 * radius + 1);
    hipLaunchKernelGGL(k_displace, dim3(max_tiles, 1, count), dim3(kDispThreads), 0, st, d_qs, radius, tile_tables, tiles_off);
    hipLaunchKernelGGL(k_displace_fold, dim3((S2 + kDispThreads - 1) / kDispThreads, std::min(max_tiles, kDispFoldChunks), count), dim3(kDispThreads), 0, st,
                       d_qs, S2, tile_tables, tables);
}

}  // namespace musica
