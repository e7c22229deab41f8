// kernels_codec.hip — the lossy block codec of a dense, row-major n x n plane of u16 (the alteration source into one image of the input
// buffer: musica_alter_codec) or u8 (one reference slot into another: musica_sim_codec_reference). metrics.block_codec states it: the
// plane lies on a grid of 8 x 8 blocks that start at x = -ox, y = -oy (mod 8); a block that sticks out of the plane is completed by edge
// replication and only in-plane pixels are written. Per block, all in int32, rs(t, s) = (t + 2^(s - 1)) >> s (arithmetic):
//   X  = v - 2^(bits - 1)
//   A  = rs(X M^T, 10)                 rows        |X M^T| <= 2^27
//   F  = rs(M A, 11)                   columns     |M A| <= 2^29, |F| <= 2^18
//   q  = sign(F) ((|F| + (Q >> 1)) div Q),  F' = q Q        |F'| <= 2^18 + 32767
//   A' = clamp(rs(M^T F', 10), -2^18, 2^18 - 1)             |M^T F'| <= 3825 (2^18 + 32767) < 2^31
//   X' = rs(A' M, 11)                                       |A' M| <= 2^30
//   out = clamp(X' + 2^(bits - 1), 0, 2^bits - 1)
// with M the 8 x 8 integer DCT matrix of codec_m below (M[0][x] = 512, M[u][x] = rint(512 sqrt 2 cos((2x + 1) u pi / 16))).
//
// k_codec<T, WIDE>: a workgroup of 256 threads owns 64 x 32 pixels of the block grid: 8 x 4 blocks, 8 lanes a block, a lane a block row.
// The 8 blocks of a wavefront lie side by side, so its lanes with the same row read 128 consecutive bytes of u16 pixels.
//   load     a lane takes the 8 pixels of its row: one 16-byte load where the launcher found the plane aligned (u16, origin 0, n % 8 == 0,
//            16-byte aligned planes: every block then lies inside the plane), else 8 loads at clamped coordinates (the edge replication);
//   rows     the 1-D transform of the row in registers, folded by M's symmetry M[u][7 - x] = (-1)^u M[u][x]: the sums x + (7 - x) feed
//            the even u, the differences the odd u, 32 multiplies a row in place of 64;
//   turn     the 8 x 8 of a block is transposed among its 8 lanes, so that a lane holds a column: through the block's own 8 x 9 words
//            of LDS, 8 writes and 8 reads a lane behind a wavefront barrier (the odd pitch keeps the 8 lanes of a block on 8 banks, the
//            blocks of a wavefront 72 words apart); 9216 B a workgroup. A form that swapped one bit of the lane number with one bit of
//            the register number a step by DPP moves touched no memory but took 25.7 us at 3072^2 where this one takes 19.8 (the plain
//            copy 13.2) and was not kept: DESIGN.md section 4;
//   columns  the same transform down the column, then the quantiser: a lane holds column u and reads Q[v][u], v = 0 .. 7, once;
//            plain 32-bit unsigned division;
//   back     the transposed transform (even and odd u summed apart, x and 7 - x from their sum and difference) up the column with the
//            clamp, the turn again, then along the row; a 16-byte store or 8 bounds-checked stores.
// No float, no atomics, no scratch. Nothing outside the two planes is read or written; the planes must not overlap.
#include <type_traits>

#include "kernels_common.h"
#include "launchers.h"

namespace musica {

constexpr int kCodecThreads = 256;
constexpr int kCodecTileW = 64, kCodecTileH = 32;   // 8 x 4 blocks: 32 blocks of 8 lanes

__host__ __device__ constexpr int codec_m(int u, int x) {
    constexpr int m[8][8] = {{512, 512, 512, 512, 512, 512, 512, 512},     {710, 602, 402, 141, -141, -402, -602, -710},
                             {669, 277, -277, -669, -669, -277, 277, 669}, {602, -141, -710, -402, 402, 710, 141, -602},
                             {512, -512, -512, 512, 512, -512, -512, 512}, {402, -710, 141, 602, -602, -141, 710, -402},
                             {277, -669, 669, -277, -277, 669, -669, 277}, {141, -402, 602, -710, 710, -602, 402, -141}};
    return m[u][x];
}
constexpr bool codec_m_folds() {
    for (int u = 0; u < 8; u++)
        for (int x = 0; x < 4; x++)
            if (codec_m(u, 7 - x) != ((u & 1) ? -codec_m(u, x) : codec_m(u, x))) return false;
    return true;
}
static_assert(codec_m_folds(), "M[u][7 - x] = (-1)^u M[u][x]: what the folded passes rely on");

template <int S>
__device__ __forceinline__ int codec_rs(int t) { return (t + (1 << (S - 1))) >> S; }

// out[u] = rs(sum_x M[u][x] in[x], S)
template <int S>
__device__ __forceinline__ void codec_forward(int (&v)[8]) {
    int s[4], d[4];
#pragma unroll
    for (int x = 0; x < 4; x++) {
        s[x] = v[x] + v[7 - x];
        d[x] = v[x] - v[7 - x];
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
        int t = 0;
#pragma unroll
        for (int x = 0; x < 4; x++) t += codec_m(u, x) * ((u & 1) ? d[x] : s[x]);
        v[u] = codec_rs<S>(t);
    }
}

// out[x] = rs(sum_u M[u][x] in[u], S), clamped to 19 bits where CLAMP
template <int S, bool CLAMP>
__device__ __forceinline__ void codec_inverse(int (&v)[8]) {
    int e[4], o[4];
#pragma unroll
    for (int x = 0; x < 4; x++) {
        e[x] = o[x] = 0;
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            e[x] += codec_m(u, x) * v[u];
            o[x] += codec_m(u + 1, x) * v[u + 1];
        }
    }
#pragma unroll
    for (int x = 0; x < 4; x++) {
        v[x] = codec_rs<S>(e[x] + o[x]);
        v[7 - x] = codec_rs<S>(e[x] - o[x]);
    }
    if (CLAMP) {
#pragma unroll
        for (int x = 0; x < 8; x++) v[x] = min(max(v[x], -(1 << 18)), (1 << 18) - 1);
    }
}

// v[i] of lane l (of its 8) becomes v[l] of lane i, through `block`: the block's own 8 x 9 words of LDS, written and read only by its
// own 8 lanes, which share a wavefront. All 64 lanes of the wavefront are active.
__device__ __forceinline__ void codec_turn(int (&v)[8], int lane8, int* __restrict__ block) {
#pragma unroll
    for (int i = 0; i < 8; i++) block[lane8 * 9 + i] = v[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = block[i * 9 + lane8];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T, bool WIDE>
__global__ __launch_bounds__(kCodecThreads) void k_codec(const T* __restrict__ src, T* __restrict__ out, int n, int origin, CodecTable table) {
    static_assert(!WIDE || sizeof(T) == 2, "the 16-byte path is the u16 plane's");
    constexpr int BITS = 8 * (int)sizeof(T), HALF = 1 << (BITS - 1), TOP = (1 << BITS) - 1;
    __shared__ int turn[kCodecThreads / 8 * 72];
    const int t = threadIdx.x, lane8 = t & 7, block = t >> 3;     // block: 8 a wavefront, side by side; 4 wavefronts below each other
    const int gx = (int)blockIdx.x * kCodecTileW + (block & 7) * 8;               // the block's place on the grid
    const int gy = (int)blockIdx.y * kCodecTileH + (block >> 3) * 8 + lane8;      // the lane's row on the grid
    const int px = gx - origin, py = gy - origin;                                 // in the plane; outside it where the grid overhangs
    int* mine = turn + block * 72;

    // A block wholly outside the plane (beyond the last column or row of blocks) still runs: its lanes read clamped pixels and write
    // nothing, so every lane of the wavefront reaches the turns.
    int v[8];
    if (WIDE) {   // origin 0, n % 8 == 0: a block lies inside the plane or wholly outside it
        union {
            uint4 w;
            uint16_t p[8];
        } row;
        row.w = *reinterpret_cast<const uint4*>(src + (size_t)min(py, n - 1) * n + min(px, n - 8));
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = (int)row.p[i] - HALF;
    } else {
        const T* line = src + (size_t)min(max(py, 0), n - 1) * n;
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = (int)line[min(max(px + i, 0), n - 1)] - HALF;
    }

    codec_forward<10>(v);            // A[y][u], y the lane
    codec_turn(v, lane8, mine);   // A[y][u], u the lane
    codec_forward<11>(v);            // F[v][u]
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t q = table.q[i * 8 + lane8];
        const uint32_t mag = ((uint32_t)abs(v[i]) + (q >> 1)) / q * q;   // <= 2^18 + 32767
        v[i] = v[i] < 0 ? -(int)mag : (int)mag;
    }
    codec_inverse<10, true>(v);      // A'[y][u], u the lane
    codec_turn(v, lane8, mine);   // y the lane again
    codec_inverse<11, false>(v);     // X'[y][x]

    if (py < 0 || py >= n) return;
    if (WIDE) {
        if (px >= n) return;
        union {
            uint4 w;
            uint16_t p[8];
        } row;
#pragma unroll
        for (int i = 0; i < 8; i++) row.p[i] = (uint16_t)min(max(v[i] + HALF, 0), TOP);
        *reinterpret_cast<uint4*>(out + (size_t)py * n + px) = row.w;
    } else {
        T* line = out + (size_t)py * n;
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (px + i >= 0 && px + i < n) line[px + i] = (T)min(max(v[i] + HALF, 0), TOP);
    }
}

template <typename T, bool WIDE>
static void launch_codec_as(hipStream_t st, const T* src, T* out, int n, int origin, const CodecTable& table) {
    const dim3 grid((unsigned)((n + origin + kCodecTileW - 1) / kCodecTileW), (unsigned)((n + origin + kCodecTileH - 1) / kCodecTileH));
    hipLaunchKernelGGL((k_codec<T, WIDE>), grid, dim3(kCodecThreads), 0, st, src, out, n, origin, table);
}

void launch_codec_u16(hipStream_t st, const uint16_t* src, uint16_t* out, int n, int origin, const CodecTable& table) {
    const bool wide = origin == 0 && n % 8 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    if (wide) launch_codec_as<uint16_t, true>(st, src, out, n, origin, table);
    else launch_codec_as<uint16_t, false>(st, src, out, n, origin, table);
}

void launch_codec_u8(hipStream_t st, const uint8_t* src, uint8_t* out, int n, int origin, const CodecTable& table) {
    launch_codec_as<uint8_t, false>(st, src, out, n, origin, table);
}

}  // namespace musica
