// study_device.h — what the study's kernels share on the device (kernels_similarity.hip, kernels_scales.hip, kernels_joint.hip,
// kernels_displace.hip, kernels_covariance.hip, kernels_ensemble.hip): the address-space typedefs, the reductions and their ONE order,
// the 64 x 64 tile of a region, the packed byte windows of k_displace and k_cov_add, and the per-window SSIM terms.
#pragma once

#include "kernels_common.h"
#include "launchers.h"

namespace musica {

static_assert(kSimTile == MUSICA_SIM_TILE && kSimMaxRadius == MUSICA_SIM_MAX_RADIUS, "the study kernels' tiles and radii are include/musica.h's");

constexpr int kStudyThreads = 256;                 // every study kernel that reduces over its workgroup has this many threads
constexpr int kStudyWaves = kStudyThreads / 64;

// The planes are device memory: say so, or the pointers read from a query are generic and the loads come out as flat_load.
typedef __attribute__((address_space(1))) float GlobalF32;
typedef __attribute__((address_space(1))) uint8_t GlobalU8;
typedef __attribute__((address_space(1))) unsigned long long GlobalU64;

__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }

// ---- reductions ----------------------------------------------------------------------------------------------------------------------
// THE ORDER RULE. A value is reduced over a workgroup in one fixed order: inside a wavefront by the __shfl_down tree 32, 16 .. 1 (lane 0
// ends with the wavefront's value), then the wavefronts 0 .. kStudyWaves - 1 in ascending order by thread 0, which alone holds the
// result. f64 addition is not associative: this order, with per-workgroup partials folded by a second kernel in the same way instead of
// f64 atomics, is why the study's doubles are bit-identical from call to call. Integer sums, minima and maxima take the same path.
// Sums every argument over its wavefront, in place: ONE loop over the offsets for all of them, so that their shuffle trees interleave
// instead of running one dependent chain after the other.
template <typename... T>
__device__ __forceinline__ void wave_sum(T&... v) {
    for (int off = 32; off > 0; off >>= 1) ((v += __shfl_down(v, off, 64)), ...);
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ bool wave_leader() { return (threadIdx.x & 63) == 0; }

// The wavefronts' values of N reduced quantities of one type, in LDS. The caller reduces ALL its values over the wavefront first, then
// stores them in ONE `if (wave_leader())` block with put() (one predicated region, stores that merge), places ONE __syncthreads() behind
// it, and thread 0 reads sum(i) / min(i) / max(i).
template <typename T, int N = 1>
struct WaveSlots {
    T w[kStudyWaves][N];
    __device__ __forceinline__ void put(const T (&v)[N]) {   // wave leaders only
#pragma unroll
        for (int i = 0; i < N; i++) w[threadIdx.x >> 6][i] = v[i];
    }
    __device__ __forceinline__ void put(T v) {                // wave leaders only
        static_assert(N == 1, "one value for one quantity");
        w[threadIdx.x >> 6][0] = v;
    }
    __device__ __forceinline__ T sum(int i = 0) const {
        T r = w[0][i];
        for (int k = 1; k < kStudyWaves; k++) r += w[k][i];
        return r;
    }
    __device__ __forceinline__ T min(int i = 0) const {
        T r = w[0][i];
        for (int k = 1; k < kStudyWaves; k++) r = w[k][i] < r ? w[k][i] : r;
        return r;
    }
    __device__ __forceinline__ T max(int i = 0) const {
        T r = w[0][i];
        for (int k = 1; k < kStudyWaves; k++) r = w[k][i] > r ? w[k][i] : r;
        return r;
    }
};

// ---- tiles ---------------------------------------------------------------------------------------------------------------------------
// Tile `tile` (tile-row major) of a w x h region cut into kSimTile^2 tiles from its origin: where it starts and how much of it lies
// inside the region (the last tile of a row or column is ragged).
struct TileGeom {
    int x0, y0, tw, th;
};
__device__ __forceinline__ TileGeom tile_geom(int tile, int tiles_x, int w, int h) {
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x0 = tx * kSimTile, y0 = ty * kSimTile;
    return {x0, y0, min(kSimTile, w - x0), min(kSimTile, h - y0)};
}

// ---- packed byte windows (k_displace, k_cov_add) -------------------------------------------------------------------------------------
// Both kernels hold a tile as packed bytes, 16 words per row at a 16-byte aligned pitch, and the window their candidates / lags reach
// as packed bytes from byte 0 of each row. A work item is (candidate or lag, block of kByteRows tile rows), dealt to the threads
// round-robin with the candidate fastest, so the lanes of a wavefront hold neighbouring dx of one or two dy and read the same 16 B of
// the tile row (an LDS broadcast); per 16 pixels an item reads those 16 B and four new words of the window row (the fifth is carried).
// Banks: ds_read_b32 banks are word % 32 over 32-lane groups. 32 neighbouring dx span at most 9 words of a window row (33 dx) and rows
// one apart are kByteWinPitch % 32 = 9 banks apart, so the groups of R >= 3 are conflict-free; lanes with equal words broadcast.
constexpr int kByteRows = 8;          // tile rows of a work item
constexpr int kByteTilePitch = 20;    // words per LDS row of the tile (16 used)
constexpr int kByteWinWords = 25;     // words per LDS row of the window that are staged: 64 + 2 * 16 + 3 bytes, rounded up
constexpr int kByteWinPitch = 41;     // words per LDS row of the window

// n >= 1 consecutive graded f32 at p (4-byte aligned), quantised with out_u8, as one word: pixel k in byte k. The first four when
// n >= 4 (one 16-byte load), else the n of a ragged tail with the bytes above them 0.
__device__ __forceinline__ uint32_t load_quant4(const GlobalF32* p, int n) {
    if (n >= 4) {
        float v[4];
        __builtin_memcpy(v, p, 16);
        return out_u8(v[0]) | (out_u8(v[1]) << 8) | (out_u8(v[2]) << 16) | (out_u8(v[3]) << 24);
    }
    uint32_t word = 0u;
    for (int k = 0; k < n; k++) word |= out_u8(p[k]) << (8 * k);
    return word;
}

// The four words of 16 window pixels shifted by sh bytes (v_alignbyte_b32): lo is the word before b1 .. b4, sh = (dx + R) & 3 with the
// word offset (dx + R) >> 2 already in the row pointer, one alignment per lane for a whole item.
__device__ __forceinline__ void shifted_words(uint32_t lo, uint32_t b1, uint32_t b2, uint32_t b3, uint32_t b4, uint32_t sh, uint32_t (&v)[4]) {
    v[0] = __builtin_amdgcn_alignbyte(b1, lo, sh);
    v[1] = __builtin_amdgcn_alignbyte(b2, b1, sh);
    v[2] = __builtin_amdgcn_alignbyte(b3, b2, sh);
    v[3] = __builtin_amdgcn_alignbyte(b4, b3, sh);
}

// ---- SSIM ----------------------------------------------------------------------------------------------------------------------------
// harness.ssim_similarity's terms of one 7 x 7 window from its means, in its order (-ffp-contract=off): ssim = (a1 a2) / (b1 b2),
// contrast-structure a2 / b2, luminance a1 / b1.
struct SsimTerms {
    double a1, a2, b1, b2;
};
__device__ __forceinline__ SsimTerms ssim_terms(double ux, double uy, double uxx, double uyy, double uxy, const SimConsts& k) {
    const double vx = k.cov_norm * (uxx - ux * ux), vy = k.cov_norm * (uyy - uy * uy), vxy = k.cov_norm * (uxy - ux * uy);
    return {2.0 * ux * uy + k.c1, 2.0 * vxy + k.c2, ux * ux + uy * uy + k.c1, vx + vy + k.c2};
}

}  // namespace musica
