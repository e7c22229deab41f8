// kernels_ensemble.hip — ensemble noise statistics of the study (musica_sim_ensemble_*, include/musica.h; harness.py
// ensemble_statistics): per pixel of the cropped (N - 20)^2 output plane the context keeps S1 = sum_k a_k and S2 = sum_k a_k^2 over the
// K <= 1024 realisations added so far (a_k: the 8-bit output of realisation k, the graded f32 plane quantised with out_u8 while it is
// read, exactly musica_get_out_pixels' bytes), packed as one 8-byte word {S1, S2} per pixel, dense rows of N - 20 words.
//
// k_ens_add: a streaming kernel. A thread owns 4 consecutive pixels of one cropped row. The run starts MUSICA_OUT_MARGIN = 10 floats into
//   a graded row whose start is 16-byte aligned (the pitch is a multiple of 4 floats) and 4 x floats further per lane: on an 8-byte
//   boundary, so it is read as two 8-byte loads per image. The thread loops over the `count` graded planes, sums a and a^2 in registers
//   and does ONE read-modify-write of its four accumulator words: no atomics, a pixel has one owner. Per pixel 4 count bytes are read and
//   16 bytes are read and written. A row of accumulator words starts on an 8-byte boundary (N - 20 may be odd), so the four words are
//   written as 8-byte accesses; gfx950's unaligned access mode lets the compiler merge them, and the two 8-byte loads of a plane, into
//   16-byte instructions. The last lane of a row whose width is no multiple of 4 reads and writes only its own pixels.
// k_ens_stats: one workgroup of 256 threads per 64 x 64 tile (MUSICA_SIM_TILE, anchored at the region's origin) and query, the query in
//   blockIdx.z as in k_sim. With b the reference slot's byte and K the realisations, per region pixel, in 64-bit integers,
//     D = S1 - K b,  V = K S2 - S1^2,  E = S2 - 2 b S1 + K b^2  (== sum_k (a_k - b)^2),
//   and the workgroup reduces sum D^2, sum V, sum D, sum E, max |D|, max V (shuffles inside a wavefront, LDS across the four). It writes
//   the tile's pair (sum D^2, sum V) and adds its sums to the query's totals with 64-bit integer atomics (add, max): exact, and the same
//   from call to call whatever the order. Every sum fits u64: musica_sim_ensemble_result refuses 65025 K^2 w h >= 2^64. No f64.
#include "study_device.h"

namespace musica {

static_assert((MUSICA_OUT_MARGIN & 1) == 0, "k_ens_add reads the cropped rows as 8-byte pairs: the margin must be even");

constexpr int kEnsThreads = kStudyThreads;

__global__ __launch_bounds__(kEnsThreads) void k_ens_add(const float* __restrict__ graded, int pitch, size_t plane, int count, int nw, int lanes_per_row,
                                                         uint2* __restrict__ acc) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = idx / lanes_per_row;
    if (y >= nw) return;
    const int x0 = (idx - y * lanes_per_row) * 4;
    const float* src = graded + (size_t)(y + MUSICA_OUT_MARGIN) * pitch + MUSICA_OUT_MARGIN + x0;
    uint2* dst = acc + (size_t)y * nw + x0;
    uint32_t s1[4] = {0u, 0u, 0u, 0u}, s2[4] = {0u, 0u, 0u, 0u};
    if (x0 + 4 > nw) {   // ragged tail of the row: 1 .. 3 pixels
        const int n = nw - x0;
        for (int k = 0; k < count; k++)
            for (int j = 0; j < n; j++) {
                const uint32_t a = out_u8(src[(size_t)k * plane + j]);
                s1[j] += a;
                s2[j] += a * a;
            }
        for (int j = 0; j < n; j++) {
            uint2 v = dst[j];
            v.x += s1[j];
            v.y += s2[j];
            dst[j] = v;
        }
        return;
    }
#pragma unroll 4
    for (int k = 0; k < count; k++) {
        const float2* s = reinterpret_cast<const float2*>(src + (size_t)k * plane);
        const float2 lo = s[0], hi = s[1];
        const uint32_t a[4] = {out_u8(lo.x), out_u8(lo.y), out_u8(hi.x), out_u8(hi.y)};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            s1[j] += a[j];
            s2[j] += a[j] * a[j];
        }
    }
    uint2 v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = dst[j];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v[j].x += s1[j];
        v[j].y += s2[j];
        dst[j] = v[j];
    }
}

__global__ __launch_bounds__(kEnsThreads) void k_ens_stats(const EnsQueryDev* __restrict__ qs, uint32_t K, unsigned long long* __restrict__ tile_tables,
                                                           unsigned long long* __restrict__ totals) {
    __shared__ WaveSlots<unsigned long long, kEnsTotals> part;
    const EnsQueryDev q = qs[blockIdx.z];
    const int tile = blockIdx.x;
    if (tile >= q.tiles_x * q.tiles_y) return;   // whole workgroup: the grid is sized for the query with the most tiles
    const int t = threadIdx.x;
    const auto [x0, y0, tw, th] = tile_geom(tile, q.tiles_x, q.w, q.h);
    // one accumulator word: S1 in the low half, S2 in the high one
    const GlobalU64* __restrict__ ps = (const GlobalU64*)q.s + (ptrdiff_t)y0 * q.s_pitch + x0;
    const GlobalU8* __restrict__ pb = (const GlobalU8*)q.b + (ptrdiff_t)y0 * q.b_pitch + x0;
    const long long k = (long long)K;
    unsigned long long sq_bias = 0ull, var = 0ull, sq_err = 0ull, bias_max = 0ull, var_max = 0ull;
    long long bias = 0ll;
    for (int i = t; i < kSimTile * kSimTile; i += kEnsThreads) {
        const int r = i >> 6, x = i & 63;
        if (r >= th || x >= tw) continue;
        const unsigned long long s = ps[(ptrdiff_t)r * q.s_pitch + x];
        const long long s1 = (long long)(s & 0xFFFFFFFFull), s2 = (long long)(s >> 32), b = (long long)pb[(ptrdiff_t)r * q.b_pitch + x];
        const long long d = s1 - k * b;
        const unsigned long long v = (unsigned long long)(k * s2 - s1 * s1);   // >= 0 (Cauchy-Schwarz)
        const unsigned long long ad = (unsigned long long)(d < 0 ? -d : d);
        sq_bias += ad * ad;
        var += v;
        bias += d;
        sq_err += (unsigned long long)(s2 - 2 * b * s1 + k * b * b);           // >= 0: a sum of squares
        bias_max = ad > bias_max ? ad : bias_max;
        var_max = v > var_max ? v : var_max;
    }
    unsigned long long ubias = (unsigned long long)bias;   // two's complement: the wrapped sum is the signed one
    wave_sum(sq_bias);
    wave_sum(var);
    wave_sum(ubias);
    wave_sum(sq_err);
    const unsigned long long wave[kEnsTotals] = {sq_bias, var, ubias, sq_err, wave_max(bias_max), wave_max(var_max)};
    if (wave_leader()) part.put(wave);
    __syncthreads();
    if (t == 0) {
        unsigned long long r[kEnsTotals];
        for (int j = 0; j < 4; j++) r[j] = part.sum(j);
        for (int j = 4; j < kEnsTotals; j++) r[j] = part.max(j);
        unsigned long long* pair = tile_tables + 2 * (q.tile_base + (size_t)tile);
        pair[0] = r[0];
        pair[1] = r[1];
        unsigned long long* out = totals + (size_t)blockIdx.z * kEnsTotals;
        for (int j = 0; j < 4; j++) atomicAdd(&out[j], r[j]);
        for (int j = 4; j < kEnsTotals; j++) atomicMax(&out[j], r[j]);
    }
}

void launch_ens_add(hipStream_t st, const float* graded, const LevelDesc& l0, int count, uint2* acc) {
    const int nw = l0.S - 2 * MUSICA_OUT_MARGIN;
    const int lanes_per_row = (nw + 3) / 4;
    const dim3 grid((unsigned)(((size_t)nw * lanes_per_row + kEnsThreads - 1) / kEnsThreads));
    hipLaunchKernelGGL(k_ens_add, grid, dim3(kEnsThreads), 0, st, graded, l0.pitch, l0.plane, count, nw, lanes_per_row, acc);
}

void launch_ens_stats(hipStream_t st, const EnsQueryDev* d_qs, int count, int max_tiles, uint32_t K, unsigned long long* tile_tables,
                      unsigned long long* totals) {
    hipLaunchKernelGGL(k_ens_stats, dim3(max_tiles, 1, count), dim3(kEnsThreads), 0, st, d_qs, K, tile_tables, totals);
}

}  // namespace musica
