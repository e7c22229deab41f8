// kernels_covariance.hip — the spatial auto-covariance of the output noise over an ensemble (musica_sim_ensemble_track / _covariance,
// include/musica.h; harness.py ensemble_covariance). a_k(p) is the 8-bit output of realisation k (the graded f32 plane quantised with
// out_u8 while it is read, exactly what k_ens_add adds), a tracked region is a rectangle of the cropped (N - 20)^2 plane, the lags are
// d = (dx, dy), dy = 0 .. R, dx = -R .. R: T = (R + 1) S entries, S = 2 R + 1, row dy, column dx + R. Per 64 x 64 tile of the region
// (anchored at the region's origin, ragged last tiles) the context keeps P(d) = sum_k sum_p a_k(p) a_k(p + d) as u64; at result time
// U(d) = sum_p S1(p) S1(p + d) comes from the ensemble's accumulators and C(d) = K P(d) - U(d).
//
// k_cov_add: one workgroup of 256 threads per (tile, region), the region in blockIdx.z. ACCUMULATION SCHEME: the workgroup owns its tile
//   across the realisations of the launch. It loops over the `count` graded planes, keeps the tile's u64 sums in registers (T <= 561
//   entries, at most 3 per thread) and ends with ONE plain read-modify-write of its tile table: no global atomics, a tile has one owner,
//   launches on one stream follow each other.
//   * Staging, per realisation (the layout, the work items and the bank argument: study_device.h, packed byte windows; they are
//     k_displace's). The window the tile's lags reach, (tile_w + 2 R) x (tile_h + R) pixels from (64 tx - R, 64 ty) of the region, goes
//     into LDS from byte 0 of each row, quantised once. Bytes past the window are 0 and never loaded: musica_sim_ensemble_track refuses
//     a region whose grown window leaves the plane, so everything that is loaded lies inside it. The tile itself (the window from byte R
//     of each row on) is then copied inside LDS into the tile's rows with v_alignbyte_b32; pixels at x >= tile_w of a ragged tile are
//     cleared there.
//   * There are T * ceil(tile_h / 8) work items. Per 16 pixels an item forms the four shifted words and does four v_dot4_u32_u8: 0.25
//     instructions per pixel and lag, half of k_displace's.
//   * Padding. Rows past tile_h are not visited. A pixel is masked by ITS position in the region (the tile copy holds 0 at x >= tile_w, so
//     the products of a padded pixel are 0 for every lag), never by where its partner lies: a pixel inside the region does see partners
//     beyond the region's edge.
//   * Ranges. An item's sum is <= 8 * 64 * 255^2 < 2^25 and goes to its lag's entry of an LDS table with one integer LDS atomic; an entry
//     is at most 64 * 64 * 255^2 = 266 342 400 < 2^28 per realisation. The u32 table is flushed into the u64 registers after EVERY
//     realisation (16 would still fit, 17 would not).
// k_cov_mean: the same tiling over the accumulator words. The S1 window, (64 + 32) x (64 + 16) u32 = 30 KiB (row pitch 97 words: lanes
//   hold consecutive dx, rows of neighbouring dy then lie 1 bank apart), S1 <= 261 120, so an item does 32 x 32 -> 64-bit multiply-adds,
//   <= 8 * 64 * 261120^2 < 2^46, into a u64 LDS table (a tile's U < 2^48). The tile's C(d) = K P(d) - U(d) is written as i64 and added to
//   the region's table with one 64-bit integer atomic per lag: the wrapped two's-complement sum is the signed one (as k_ens_stats' bias_sum).
// Everything is integer arithmetic: exact, and the same from call to call whatever the order. No f64.
#include "study_device.h"

namespace musica {

constexpr int kCovThreads = kStudyThreads;
constexpr int kCovWinRows = kSimTile + kSimMaxRadius;        // 80
constexpr int kCovMaxLags = (kSimMaxRadius + 1) * (2 * kSimMaxRadius + 1);   // 561
constexpr int kCovPerThread = (kCovMaxLags + kCovThreads - 1) / kCovThreads; // 3
constexpr int kCovMeanCols = kSimTile + 2 * kSimMaxRadius;   // 96
constexpr int kCovMeanPitch = 97;

__global__ __launch_bounds__(kCovThreads) void k_cov_add(const CovRegionDev* __restrict__ rs, int radius, const float* __restrict__ graded, int pitch,
                                                         size_t plane, int count, unsigned long long* __restrict__ tile_tables) {
    __shared__ __attribute__((aligned(16))) uint32_t sa[kSimTile * kByteTilePitch];
    __shared__ uint32_t sw[kCovWinRows * kByteWinPitch];
    __shared__ uint32_t tab[kCovMaxLags];
    const CovRegionDev q = rs[blockIdx.z];
    const int tile = blockIdx.x;
    if (tile >= q.tiles_x * q.tiles_y) return;   // whole workgroup: the grid is sized for the region with the most tiles
    const int t = threadIdx.x;
    const auto [x0, y0, tw, th] = tile_geom(tile, q.tiles_x, q.w, q.h);
    const int S = 2 * radius + 1, T = (radius + 1) * S;
    const int bw = tw + 2 * radius, bh = th + radius;   // the window in bytes and rows: inside the plane (the call's refusals)
    const int blocks = (th + kByteRows - 1) / kByteRows;
    const int full = tw >> 4, rest = tw & 15;
    const uint32_t ash = (uint32_t)(radius & 3);
    const int aw = radius >> 2;
    for (int i = t; i < T; i += kCovThreads) tab[i] = 0u;
    unsigned long long acc[kCovPerThread] = {};
    // the window's first pixel in a graded plane: column ax + x0 - radius, row ay + y0 of the cropped plane
    const ptrdiff_t origin = (ptrdiff_t)(q.ay + y0 + MUSICA_OUT_MARGIN) * pitch + (q.ax + x0 - radius + MUSICA_OUT_MARGIN);

    for (int k = 0; k < count; k++) {
        const GlobalF32* __restrict__ pw = (const GlobalF32*)graded + (size_t)k * plane + origin;
        for (int i = t; i < bh * kByteWinWords; i += kCovThreads) {
            const int r = i / kByteWinWords, wd = i - r * kByteWinWords, j = wd << 2;
            sw[r * kByteWinPitch + wd] = j < bw ? load_quant4(pw + (ptrdiff_t)r * pitch + j, bw - j) : 0u;
        }
        __syncthreads();
        // the tile: the window from byte `radius` of each row on, 16 words per row; bytes at x >= tw cleared (words aw + wd + 1 <= 4 + 15 + 1 < 25)
        for (int i = t; i < th * 16; i += kCovThreads) {
            const int r = i >> 4, wd = i & 15, n = tw - (wd << 2);
            const uint32_t* row = sw + r * kByteWinPitch + aw + wd;
            const uint32_t v = __builtin_amdgcn_alignbyte(row[1], row[0], ash);
            sa[r * kByteTilePitch + wd] = n >= 4 ? v : n <= 0 ? 0u : v & ((1u << (8 * n)) - 1u);
        }
        __syncthreads();

        for (int i = t; i < T * blocks; i += kCovThreads) {
            const int p = i / T, c = i - p * T;
            const int dy = c / S, dxi = c - dy * S;   // dy, dx + R
            const uint32_t sh = (uint32_t)(dxi & 3);
            const int y1 = min(th, (p + 1) * kByteRows);
            uint32_t sab = 0u;   // <= 8 * 64 * 255^2 < 2^25
            for (int y = p * kByteRows; y < y1; y++) {
                const uint4* ar = reinterpret_cast<const uint4*>(sa + y * kByteTilePitch);
                const uint32_t* br = sw + (y + dy) * kByteWinPitch + (dxi >> 2);
                uint32_t lo = br[0];
                const int chunks = full + (rest ? 1 : 0);   // the tile copy is 0 at x >= tw: a ragged chunk needs no mask of its own; words up to (dxi >> 2) + 16 <= 24
                for (int ch = 0; ch < chunks; ch++) {
                    const uint4 av = ar[ch];
                    const uint32_t b1 = br[4 * ch + 1], b2 = br[4 * ch + 2], b3 = br[4 * ch + 3], b4 = br[4 * ch + 4];
                    uint32_t v[4];
                    shifted_words(lo, b1, b2, b3, b4, sh, v);
                    sab = dot4(av.x, v[0], sab);
                    sab = dot4(av.y, v[1], sab);
                    sab = dot4(av.z, v[2], sab);
                    sab = dot4(av.w, v[3], sab);
                    lo = b4;
                }
            }
            atomicAdd(&tab[c], sab);
        }
        __syncthreads();
        // the u32 stage into the u64 registers, every realisation; the next realisation's staging and atomics lie behind two barriers
#pragma unroll
        for (int j = 0; j < kCovPerThread; j++) {
            const int c = t + j * kCovThreads;
            if (c < T) {
                acc[j] += tab[c];
                tab[c] = 0u;
            }
        }
    }

    GlobalU64* __restrict__ out = (GlobalU64*)tile_tables + q.tile_base + (size_t)tile * T;
#pragma unroll
    for (int j = 0; j < kCovPerThread; j++) {
        const int c = t + j * kCovThreads;
        if (c < T) out[c] += acc[j];
    }
}

__global__ __launch_bounds__(kCovThreads) void k_cov_mean(const CovRegionDev* __restrict__ rs, int radius, uint32_t K, const uint2* __restrict__ ens, int nw,
                                                          const unsigned long long* __restrict__ tile_tables, long long* __restrict__ tile_cov,
                                                          unsigned long long* __restrict__ tables) {
    __shared__ uint32_t s1[kCovWinRows * kCovMeanPitch];
    __shared__ unsigned long long tab[kCovMaxLags];
    const CovRegionDev q = rs[blockIdx.z];
    const int tile = blockIdx.x;
    if (tile >= q.tiles_x * q.tiles_y) return;   // whole workgroup
    const int t = threadIdx.x;
    const auto [x0, y0, tw, th] = tile_geom(tile, q.tiles_x, q.w, q.h);
    const int S = 2 * radius + 1, T = (radius + 1) * S;
    const int bw = tw + 2 * radius, bh = th + radius;   // inside the plane (the call's refusals)
    for (int i = t; i < T; i += kCovThreads) tab[i] = 0ull;
    // one accumulator word is {S1, S2}: S1 is its low half
    const GlobalU64* __restrict__ ps = (const GlobalU64*)ens + (ptrdiff_t)(q.ay + y0) * nw + (q.ax + x0 - radius);
    for (int i = t; i < bh * kCovMeanCols; i += kCovThreads) {
        const int r = i / kCovMeanCols, j = i - r * kCovMeanCols;
        s1[r * kCovMeanPitch + j] = j < bw ? (uint32_t)ps[(ptrdiff_t)r * nw + j] : 0u;
    }
    __syncthreads();

    const int blocks = (th + kByteRows - 1) / kByteRows;
    for (int i = t; i < T * blocks; i += kCovThreads) {
        const int p = i / T, c = i - p * T;
        const int dy = c / S, dxi = c - dy * S;
        const int y1 = min(th, (p + 1) * kByteRows);
        unsigned long long u = 0ull;   // <= 8 * 64 * 261120^2 < 2^46
        for (int y = p * kByteRows; y < y1; y++) {
            const uint32_t* ar = s1 + y * kCovMeanPitch + radius;
            const uint32_t* br = s1 + (y + dy) * kCovMeanPitch + dxi;
            for (int x = 0; x < tw; x++) u += (unsigned long long)ar[x] * br[x];
        }
        atomicAdd(&tab[c], u);
    }
    __syncthreads();

    const size_t base = q.tile_base + (size_t)tile * T;
    for (int c = t; c < T; c += kCovThreads) {
        const unsigned long long v = (unsigned long long)K * tile_tables[base + c] - tab[c];   // two's complement: the signed K P - U
        tile_cov[base + c] = (long long)v;
        if (v) atomicAdd(&tables[(size_t)blockIdx.z * T + c], v);
    }
}

void launch_cov_add(hipStream_t st, const CovRegionDev* d_rs, int regions, int max_tiles, int radius, const float* graded, const LevelDesc& l0, int count,
                    unsigned long long* tile_tables) {
    hipLaunchKernelGGL(k_cov_add, dim3(max_tiles, 1, regions), dim3(kCovThreads), 0, st, d_rs, radius, graded, l0.pitch, l0.plane, count, tile_tables);
}

void launch_cov_mean(hipStream_t st, const CovRegionDev* d_rs, int regions, int max_tiles, int radius, uint32_t K, const uint2* ens, int nw,
                     const unsigned long long* tile_tables, long long* tile_cov, unsigned long long* tables) {
    hipLaunchKernelGGL(k_cov_mean, dim3(max_tiles, 1, regions), dim3(kCovThreads), 0, st, d_rs, radius, K, ens, nw, tile_tables, tile_cov, tables);
}

}  // namespace musica
