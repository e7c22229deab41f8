// kernels_displace.hip — exact block matching of the study (musica_sim_displace, include/musica.h; harness.py displacement_table): the
// sum of squared differences between a region of a batch image's 8-bit output (side a: the graded f32 plane quantised with out_u8 while
// it is read, exactly what k_sim compares) and the same region of a reference slot (side b) displaced by every integer shift
// (dx, dy) in [-R, R]^2, per 64 x 64 tile of the region and, folded, for the whole region. S = 2 R + 1.
//
// k_displace: one workgroup of 256 threads per tile, the query in blockIdx.z as in k_sim.
//   * Staging. The tile of a goes into LDS as packed bytes, 16 words per row (row pitch 20 words), quantised once; pixels outside the
//     region (a ragged last tile) are 0. The window of b the tile's candidates reach, (tile_w + 2 R) x (tile_h + 2 R) bytes from
//     (64 tx - R, 64 ty - R) of the region, goes into LDS as packed bytes from byte 0 of each row (row pitch 41 words), whatever the
//     alignment of bx in the plane: the staging copy absorbs it (a word of 4 bytes from a pointer of alignment 1 is one global_load_dword
//     in gfx950's unaligned access mode). Bytes past the window are 0 and never loaded: musica_sim_displace refuses a query whose grown b
//     window leaves the plane, so everything that is loaded lies inside it.
//   * SSD = sum a^2 + sum b'^2 - 2 sum a b'. sum a^2 does not depend on the candidate and is taken once while a is staged. A work item is
//     (candidate, block of 8 tile rows): S^2 * ceil(tile_h / 8) items, dealt to the threads round-robin with the candidate fastest, so
//     the lanes of a wavefront hold neighbouring dx of one or two dy and read the same 16 B of a (an LDS broadcast). Per 16 pixels of a row
//     an item reads 16 B of a and four new words of b (the fifth is carried from the previous 16 pixels), forms the four shifted words
//     of b' with v_alignbyte_b32 (shift (dx + R) & 3 bytes, word offset (dx + R) >> 2: one alignment per lane for the whole item) and
//     does eight v_dot4_u32_u8: four for a b', four for b'^2. That is 2 multiply-adds per pixel and candidate, 0.5 dot4 instructions.
//   * Padding. Rows past tile_h are not visited. In the last, partial, 16 pixels of a ragged row b' is masked by the pixel's position in
//     the REGION (bytes at x >= tile_w are cleared after the shift), not by where its source byte lies: a padded pixel adds 0 to
//     sum a^2, sum a b' and sum b'^2 of every candidate, while a pixel inside the region sees b beyond the region's edge.
//   * Banks. ds_read_b32 banks are word % 32 over 32-lane groups. 32 neighbouring candidates span at most 9 words of a row of b (33 dx)
//     and rows one apart are 41 % 32 = 9 banks apart, so the groups of R >= 3 are conflict-free; lanes with equal words broadcast.
//   * An item adds sum b'^2 - 2 sum a b' (mod 2^32) to its candidate's entry of an LDS table with one integer LDS atomic; the entry plus
//     sum a^2 is the tile's SSD, at most 64 * 64 * 255^2 < 2^32, so the arithmetic mod 2^32 is exact. The tile table is written as u32.
//   * The tile's own argmin (smallest value, then smallest dx^2 + dy^2, then smallest dy, then smallest dx: the minimum of the 64-bit
//     key value << 32 | d^2 << 12 | (dy + R) << 6 | (dx + R)) is reduced over the workgroup; a tile whose argmin is not (0, 0) adds 1 to
//     the query's tiles_off with one integer atomic.
// k_displace_fold: the query's tile tables summed into its u64 table, a thread per candidate over a chunk of tiles, one 64-bit integer
// atomic per (candidate, chunk). Everything is integer arithmetic: exact, and the same from call to call whatever the order.
#include <algorithm>

#include "kernels_common.h"
#include "launchers.h"

namespace musica {

constexpr int kDispThreads = 256;
constexpr int kDispRows = 8;                 // tile rows of a work item
constexpr int kDispAPitch = 20;              // words per LDS row of a (16 used; 16-byte aligned rows)
constexpr int kDispBWords = 25;              // words per LDS row of b that are staged: 64 + 2 * 16 + 3 bytes, rounded up
constexpr int kDispBPitch = 41;              // words per LDS row of b
constexpr int kDispMaxS = 2 * kDisplaceMaxRadius + 1;
constexpr int kDispFoldChunks = 32;          // tile chunks of k_displace_fold
typedef __attribute__((address_space(1))) float GlobalF32;
typedef __attribute__((address_space(1))) uint8_t GlobalU8;

__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }

// 16 pixels of one row for one candidate: av the words of a, lo the word of b before b1 .. b4, sh the byte shift. `valid`: pixels of the
// 16 that lie in the region (MASK only).
template <bool MASK>
__device__ __forceinline__ void disp_chunk(const uint4 av, uint32_t lo, uint32_t b1, uint32_t b2, uint32_t b3, uint32_t b4, uint32_t sh,
                                           int valid, uint32_t& sab, uint32_t& sbb) {
    uint32_t v[4] = {__builtin_amdgcn_alignbyte(b1, lo, sh), __builtin_amdgcn_alignbyte(b2, b1, sh), __builtin_amdgcn_alignbyte(b3, b2, sh),
                     __builtin_amdgcn_alignbyte(b4, b3, sh)};
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
    __shared__ __attribute__((aligned(16))) uint32_t sa[kDisplaceTile * kDispAPitch];
    __shared__ uint32_t sb[(kDisplaceTile + 2 * kDisplaceMaxRadius) * kDispBPitch];
    __shared__ uint32_t tab[kDispMaxS * kDispMaxS];
    __shared__ uint32_t saa;
    __shared__ unsigned long long best[kDispThreads / 64];
    const DisplaceQueryDev q = qs[blockIdx.z];
    const int tile = blockIdx.x;
    if (tile >= q.tiles_x * q.tiles_y) return;   // whole workgroup: the grid is sized for the query with the most tiles
    const int t = threadIdx.x;
    const int ty = tile / q.tiles_x, tx = tile - ty * q.tiles_x;
    const int x0 = tx * kDisplaceTile, y0 = ty * kDisplaceTile;
    const int tw = min(kDisplaceTile, q.w - x0), th = min(kDisplaceTile, q.h - y0);
    const int S = 2 * radius + 1, S2 = S * S;
    for (int i = t; i < S2; i += kDispThreads) tab[i] = 0u;
    if (t == 0) saa = 0u;
    __syncthreads();

    // the planes are device memory: say so, or the pointers read from the query are generic and the loads come out as flat_load
    const GlobalF32* __restrict__ pa = (const GlobalF32*)q.a + (ptrdiff_t)y0 * q.a_pitch + x0;
    uint32_t aa = 0u;
    for (int i = t; i < kDisplaceTile * 16; i += kDispThreads) {
        const int r = i >> 4, x = (i & 15) << 2;
        uint32_t word = 0u;
        if (r < th && x < tw) {
            const GlobalF32* p = pa + (ptrdiff_t)r * q.a_pitch + x;
            if (x + 4 <= tw) {
                float v[4];
                __builtin_memcpy(v, p, 16);   // 4-byte aligned
                word = out_u8(v[0]) | (out_u8(v[1]) << 8) | (out_u8(v[2]) << 16) | (out_u8(v[3]) << 24);
            } else {
                for (int k = 0; k < tw - x; k++) word |= out_u8(p[k]) << (8 * k);
            }
        }
        sa[r * kDispAPitch + (i & 15)] = word;
        aa = dot4(word, word, aa);
    }
    for (int off = 32; off > 0; off >>= 1) aa += __shfl_down(aa, off, 64);
    if ((t & 63) == 0) atomicAdd(&saa, aa);

    const int bw = tw + 2 * radius, bh = th + 2 * radius;   // the window of b in bytes and rows: inside the plane (the call's refusals)
    const GlobalU8* __restrict__ pb = (const GlobalU8*)q.b + (ptrdiff_t)(y0 - radius) * q.b_pitch + (x0 - radius);
    for (int i = t; i < bh * kDispBWords; i += kDispThreads) {
        const int r = i / kDispBWords, wd = i - r * kDispBWords, j = wd << 2;
        uint32_t word = 0u;
        if (j < bw) {
            const GlobalU8* p = pb + (ptrdiff_t)r * q.b_pitch + j;
            if (j + 4 <= bw) {
                __builtin_memcpy(&word, p, 4);   // 1-byte aligned
            } else {
                for (int k = 0; k < bw - j; k++) word |= (uint32_t)p[k] << (8 * k);
            }
        }
        sb[r * kDispBPitch + wd] = word;
    }
    __syncthreads();

    const int blocks = (th + kDispRows - 1) / kDispRows;
    const int full = tw >> 4, rest = tw & 15;
    for (int i = t; i < S2 * blocks; i += kDispThreads) {
        const int p = i / S2, c = i - p * S2;
        const int dyi = c / S, dxi = c - dyi * S;   // dy + R, dx + R
        const uint32_t sh = (uint32_t)(dxi & 3);
        const int y1 = min(th, (p + 1) * kDispRows);
        uint32_t sab = 0u, sbb = 0u;   // <= 8 * 64 * 255^2 < 2^25
        for (int y = p * kDispRows; y < y1; y++) {
            const uint4* ar = reinterpret_cast<const uint4*>(sa + y * kDispAPitch);
            const uint32_t* br = sb + (y + dyi) * kDispBPitch + (dxi >> 2);
            uint32_t lo = br[0];
            for (int ch = 0; ch < full; ch++) {
                const uint32_t b1 = br[4 * ch + 1], b2 = br[4 * ch + 2], b3 = br[4 * ch + 3], b4 = br[4 * ch + 4];
                disp_chunk<false>(ar[ch], lo, b1, b2, b3, b4, sh, 16, sab, sbb);
                lo = b4;
            }
            if (rest) {   // full <= 3: words up to (dxi >> 2) + 16 <= 24 < kDispBWords
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
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(key, off, 64);
        key = o < key ? o : key;
    }
    if ((t & 63) == 0) best[t >> 6] = key;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kDispThreads / 64; w++) key = best[w] < key ? best[w] : key;
        if ((uint32_t)(key & 0xFFFu) != (uint32_t)((radius << 6) | radius)) atomicAdd(&tiles_off[blockIdx.z], 1u);
    }
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
