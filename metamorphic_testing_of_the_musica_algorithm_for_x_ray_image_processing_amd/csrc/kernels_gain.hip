// kernels_gain.hip — the detector-gain relation of the study (include/musica.h, musica_alter_gain / musica_sim_profiles): a separable
// gain map applied to the alteration source on its way into one image of the input buffer, and the exact row and column profiles of a
// comparison of an output against a reference slot.
//
// k_alter_gain<V>: harness.apply_gain. ONE launch, 2 B read + 2 B written per pixel, no LDS:
//   g   = gx[x] gy[y]                              both below 2^16: an exact u32 (v_mul_u32_u24)
//   out = min((v g + 2^23) >> 24, 65535)           ONE rounding, halves up; v g + 2^23 <= 65535^3 + 2^23 < 2^48
// THE 48-BIT PRODUCT IN 32-BIT WORDS. With g = 2^16 gh + gl (gh, gl < 2^16):
//   v g + 2^23 = 2^16 (v gh + 2^7) + v gl, so floor((v g + 2^23) / 2^24) = floor((v gh + 2^7 + floor(v gl / 2^16)) / 2^8):
//   floor division nests and 2^23 is a multiple of 2^16. v gh <= 65535^2 and floor(v gl / 2^16) + 128 <= 65534 + 128, so the sum stays
//   below 2^32 (asserted below): two 24-bit multiplies, two shifts and one three-operand add per pixel, no 64-bit multiply.
// A workgroup of 256 threads is four wavefronts. A lane owns V consecutive columns (study_device.h's pixel words, gx being a third
// plane of the alignment test); consecutive lanes take consecutive chunks, so a wavefront moves 1 KiB of one row per access. The lane's V entries of gx are loaded once (one 16-byte load
// for V = 8: the table is a device allocation of its own) and stay in registers while the wavefront goes down kGainRows consecutive rows,
// whose loads are all issued before the first is used. The row index comes from blockIdx.y and the wavefront's number through
// readfirstlane, so the compiler knows it is the same in every lane: gy[y] (widened to u32 by the caller, since gfx950 has no 16-bit
// scalar load) is fetched on the scalar side, once per row and wavefront, and the row's address arithmetic stays there too.
// Nothing outside the two planes and the two tables is read, nothing outside `out` written; the planes must not overlap.
//
// k_sim_profiles: harness.profile_statistics. Every query owns blockIdx.z, as in k_sim; a workgroup of 256 threads takes one 64 x 64 tile
// of the region (tile_geom). Side a is the graded f32 plane of a batch image quantised with out_u8 while it is read (load_quant4: four
// pixels, one 16-byte load; exactly what k_sim reads), side b the slot's u8 plane (four bytes, one load): 4 + 1 bytes per pixel, once.
//   lanes    16 lanes hold the 64 pixels of a tile row, so a wavefront holds 4 rows and the workgroup 16; four trips cover the tile, all
//            eight loads of a lane issued before the first is used. A lane keeps the same four columns in every trip.
//   columns  the lane's 4 columns x (sum a, sum b, sum (a - b)^2, sum a^2) stay in 16 registers over the trips; at the end the four
//            row groups of a wavefront are added with __shfl_down by 32 and by 16 (the top of wave_sum's tree), lanes 0 .. 15 put the
//            wavefront's partials into LDS and, after the barrier, thread t adds the four wavefronts' word t in ascending order.
//   rows     per trip the four sums of the lane's 4 pixels come from five v_dot4_u32_u8 (sum (a - b)^2 = a.a + b.b - 2 a.b, exact and
//            non-negative) and are reduced over the 16 lanes of the row in ONE order, 8, 4, 2, 1 lanes up; the 16 lanes are one DPP
//            row, so each step is a row_shl modifier of the add itself (row_sum below); the row's first lane puts them into LDS.
//   A lane outside the tile (a ragged last tile) holds a = b = 0 and adds 0 everywhere.
// THE COMBINATION of the tiles that share columns (tiles_y of them) or rows (tiles_x): every tile adds its 2 x 64 x 4 partials to the
// query's table, which the caller zeroes on the stream before the launch, with one u32 atomic per word and thread (no return): two
// wave-instructions of 1 KiB of contiguous words each per workgroup, 512 atomics for 4096 pixels. The sums are integers and u32
// addition commutes, so the table is exact and identical from call to call whatever order the workgroups arrive in. MEASURED
// (both forms with __shfl_down in the rows' reduction): at a 3052^2 region the launch takes what the same kernel takes
// when it stores its partials instead (22.6 us against 23.3 us), and that form needs a fold launch behind it (14.0 us as written):
// measured and not kept. With the DPP row moves the shipped launch takes 17.6 us.
// A line has at most 16364 pixels (N <= 16384): 16364 * 255^2 < 2^32, every sum fits u32 (asserted below). No float beyond out_u8's
// quantisation of side a, no f64.
#include "study_device.h"

namespace musica {

constexpr int kGainThreads = 256;
constexpr int kGainRows = 4;                                   // consecutive rows a wavefront goes down
constexpr int kGainBlockRows = kGainRows * (kGainThreads / 64);
static_assert(65535ull * 65535ull < (1ull << 32), "gx gy is an exact u32");
static_assert(65535ull * 65535ull + 65534ull + 128ull < (1ull << 32), "v gh + floor(v gl / 2^16) + 2^7 is an exact u32");
constexpr unsigned long long gain_split(unsigned long long v, unsigned long long g) { return (v * (g >> 16) + ((v * (g & 0xFFFFull)) >> 16) + 128ull) >> 8; }
static_assert(((65535ull * (65535ull * 65535ull) + (1ull << 23)) >> 24) == gain_split(65535ull, 65535ull * 65535ull) &&
                  ((65535ull * 0xFFFFFFFFull + (1ull << 23)) >> 24) == gain_split(65535ull, 0xFFFFFFFFull) && gain_split(12345ull, 4096ull * 4096ull) == 12345ull,
              "the split form at the largest intermediate, at the largest u32 and at the unit gain");

// min((v g + 2^23) >> 24, 65535) for v < 2^16: THE 48-BIT PRODUCT IN 32-BIT WORDS above
__device__ __forceinline__ uint32_t gain_pixel(uint32_t v, uint32_t g) {
    const uint32_t hi = __umul24(v, g >> 16), lo = __umul24(v, g & 0xFFFFu);
    return min((hi + (lo >> 16) + 128u) >> 8, 65535u);
}

// n % V == 0 and both planes and gx aligned to 2 V bytes; gy: the row gains widened to u32
template <int V>
__global__ __launch_bounds__(kGainThreads) void k_alter_gain(const uint16_t* __restrict__ src, uint16_t* __restrict__ out, int n,
                                                             const uint16_t* __restrict__ gx, const uint32_t* __restrict__ gy) {
    typedef typename PixelWord<V>::type __attribute__((may_alias)) Word;
    typedef PixelChunk<V> Chunk;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform: the row arithmetic stays on the scalar unit
    const int y0 = (int)blockIdx.y * kGainBlockRows + wave * kGainRows;
    const int x = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63)) * V;
    if (x >= n) return;   // a chunk starts inside the plane or lies outside it entirely (n % V == 0)
    Chunk cg;
    cg.w = *reinterpret_cast<const Word*>(gx + x);
    Chunk staged[kGainRows];
#pragma unroll
    for (int k = 0; k < kGainRows; k++)
        if (y0 + k < n) staged[k].w = *reinterpret_cast<const Word*>(src + (size_t)(y0 + k) * n + x);
#pragma unroll
    for (int k = 0; k < kGainRows; k++) {
        if (y0 + k >= n) break;   // uniform over the wavefront
        const uint32_t row = gy[y0 + k];
        Chunk v = staged[k];
#pragma unroll
        for (int i = 0; i < V; i++) v.px[i] = (uint16_t)gain_pixel(v.px[i], __umul24((uint32_t)cg.px[i], row));
        *reinterpret_cast<Word*>(out + (size_t)(y0 + k) * n + x) = v.w;
    }
}

void launch_alter_gain(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const uint16_t* d_gx, const uint32_t* d_gy) {
    launch_by_width(
        [&](auto v) {
            constexpr int V = decltype(v)::value;
            const dim3 grid((unsigned)((n / V + 63) / 64), (unsigned)((n + kGainBlockRows - 1) / kGainBlockRows));
            hipLaunchKernelGGL((k_alter_gain<V>), grid, dim3(kGainThreads), 0, st, src, out, n, d_gx, d_gy);
        },
        n, src, out, d_gx);
}

// ---- the profiles ----------------------------------------------------------------------------------------------------------------------
constexpr int kProfileLanes = kSimTile / 4;                      // lanes of a tile row, four pixels each
constexpr int kProfileRows = kStudyThreads / kProfileLanes;      // tile rows of a trip
constexpr int kProfileTrips = kSimTile / kProfileRows;
static_assert(kProfileLanes == 16 && kProfileRows == 16 && kProfileTrips == 4, "16 lanes a row, 4 rows a wavefront, 4 trips a tile");
static_assert(kSimTile * 4 == kStudyThreads, "a tile's partials: one column word and one row word per thread");
static_assert(16364ull * 255ull * 255ull < (1ull << 32), "a line's sums fit u32");

// Every argument summed over the 16 lanes of a tile row, in ONE order (8, 4, 2, 1 lanes up): the row's first lane ends with the sums.
// The 16 lanes of a tile row are one DPP row, so a lane reads the lane OFF above it in its row with row_shl (a lane whose partner
// lies beyond the row reads 0: bound_ctrl): a modifier of the add itself where __shfl_down would be a ds_bpermute_b32 each.
template <int OFF>
__device__ __forceinline__ uint32_t row_up(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 + OFF, 0xF, 0xF, true);
}
template <typename... T>
__device__ __forceinline__ void row_sum(T&... v) {
    ((v += row_up<8>(v)), ...);
    ((v += row_up<4>(v)), ...);
    ((v += row_up<2>(v)), ...);
    ((v += row_up<1>(v)), ...);
}

__global__ __launch_bounds__(kStudyThreads) void k_sim_profiles(const ProfileQueryDev* __restrict__ qs, uint32_t* __restrict__ tables) {
    __shared__ uint4 col_part[kStudyWaves][kSimTile];
    __shared__ uint4 row_part[kSimTile];
    const ProfileQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.tiles_x * q.tiles_y) return;   // whole workgroup: the grid is sized for the query with the most tiles
    const TileGeom g = tile_geom(blockIdx.x, q.tiles_x, q.w, q.h);
    const int t = threadIdx.x;
    const int cx = (t & (kProfileLanes - 1)) * 4, r = t / kProfileLanes;
    const int npx = min(4, g.tw - cx);   // <= 0: the lane's columns lie outside the tile
    const GlobalF32* pa = (const GlobalF32*)q.a + (size_t)g.y0 * q.a_pitch + (g.x0 + cx);
    const GlobalU8* pb = (const GlobalU8*)q.b + (size_t)g.y0 * q.b_pitch + (g.x0 + cx);
    uint32_t wa[kProfileTrips], wb[kProfileTrips];
#pragma unroll
    for (int k = 0; k < kProfileTrips; k++) {   // all loads first
        const int ty = k * kProfileRows + r;
        wa[k] = 0u;
        wb[k] = 0u;
        if (npx > 0 && ty < g.th) {
            wa[k] = load_quant4(pa + (size_t)ty * q.a_pitch, npx);
            wb[k] = load_bytes4(pb + (size_t)ty * q.b_pitch, npx);
        }
    }
    uint32_t ca[4] = {0u, 0u, 0u, 0u}, cb[4] = {0u, 0u, 0u, 0u}, cd[4] = {0u, 0u, 0u, 0u}, caa[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < kProfileTrips; k++) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t a = (wa[k] >> (8 * i)) & 0xFFu, b = (wb[k] >> (8 * i)) & 0xFFu;
            const uint32_t d = a > b ? a - b : b - a;
            ca[i] += a;
            cb[i] += b;
            cd[i] += d * d;
            caa[i] += a * a;
        }
        const uint32_t aa = dot4(wa[k], wa[k], 0u), ab = dot4(wa[k], wb[k], 0u);
        uint32_t ra = dot4(wa[k], 0x01010101u, 0u), rb = dot4(wb[k], 0x01010101u, 0u), rd = dot4(wb[k], wb[k], aa) - 2u * ab, raa = aa;
        row_sum(ra, rb, rd, raa);
        if ((t & (kProfileLanes - 1)) == 0) row_part[k * kProfileRows + r] = make_uint4(ra, rb, rd, raa);
    }
    // the wavefront's four row groups: lanes 0 .. 15 end with its column sums
#pragma unroll
    for (int i = 0; i < 4; i++) {
        for (int off = 32; off >= kProfileLanes; off >>= 1) {
            ca[i] += __shfl_down(ca[i], off, 64);
            cb[i] += __shfl_down(cb[i], off, 64);
            cd[i] += __shfl_down(cd[i], off, 64);
            caa[i] += __shfl_down(caa[i], off, 64);
        }
    }
    if ((t & 63) < kProfileLanes) {
#pragma unroll
        for (int i = 0; i < 4; i++) col_part[t >> 6][cx + i] = make_uint4(ca[i], cb[i], cd[i], caa[i]);
    }
    __syncthreads();
    // thread t holds word t of the tile's [64][4] column partials and of its [64][4] row partials
    const uint32_t* cw = reinterpret_cast<const uint32_t*>(&col_part[0][0]);
    uint32_t col = cw[t];
    for (int w = 1; w < kStudyWaves; w++) col += cw[w * kSimTile * 4 + t];
    const uint32_t row = reinterpret_cast<const uint32_t*>(&row_part[0])[t];
    uint32_t* ct = tables + q.table + 4 * (size_t)g.x0;
    uint32_t* rt = tables + q.table + 4 * (size_t)q.w + 4 * (size_t)g.y0;
    if ((t >> 2) < g.tw) atomicAdd(&ct[t], col);
    if ((t >> 2) < g.th) atomicAdd(&rt[t], row);
}

void launch_sim_profiles(hipStream_t st, const ProfileQueryDev* d_qs, int count, int max_tiles, uint32_t* tables) {
    hipLaunchKernelGGL(k_sim_profiles, dim3((unsigned)max_tiles, 1, (unsigned)count), dim3(kStudyThreads), 0, st, d_qs, tables);
}

}  // namespace musica
