// kernels_scatter.hip — the exact wide veiling glare of a dense, row-major n x n plane of u16 (the alteration source into one image of
// the input buffer: musica_alter_scatter) or u8 (one reference slot into another: musica_sim_scatter_reference). harness.scatter states,
// for a box radius 1 <= R <= 127 and a scatter fraction a / b (1 <= a < b <= 64, lowest terms), with
//   box(A)[i] = sum_{k = -R .. R} A[clamp(i + k)]      (clamped to the plane: edge replicated; each pass clamps its own input)
//   V   = box_y(box_y(box_x(box_x(in))))                 (tent x tent, total weight W = (2R + 1)^4)
//   out = ((b - a) W in + a V + (b W) div 2) div (b W)   (ONE rounding, after the full sum, halves up)
// Widths: after the two row passes a value is at most 255^2 * 65535 < 2^32 (the row plane is u32); W <= 255^4 < 2^32; the numerator is
// at most 65535 * 64 * 255^4 < 2^64 (the column passes and the mix are u64). Integers only: no atomics, no floats, so the four passes
// commute and the results repeat bit for bit. Two launches, both with running or prefix sums: no output costs 2R + 1 taps.
//
// k_scatter_rows<T, SH>: a workgroup of 256 threads owns ONE row, n <= 256 << SH, whole in LDS; thread t owns the segment of 1 << SH
//   consecutive elements from t << SH. SH is 0, 2, 4 or 6, the smallest that holds the row (launch_scatter), so every side up to
//   16384 is served without chunking: at SH = 6 the two u32 arrays of 16384 + 256 words and the 256 u64 segment bases take
//   2 * 66560 + 2048 + 48 = 135216 bytes, inside the 160 KiB of a workgroup; at the study's 3072 (SH = 4) 36912 bytes, four rows a CU.
//   load     the row into LDS as u32, one element per lane and trip, coalesced. Element i lives at word i + (i >> SH): one pad word a
//            segment, so the segment walks of neighbouring lanes are an odd number of banks apart for SH >= 2;
//   scan 1   inclusive, u32 (16384 * 65535 < 2^32): each thread its segment in place, the 256 segment totals by a shuffle scan per
//            wavefront and the wavefronts' totals through LDS, then the segment's offset added in place: P1;
//   box 1    B1[x] = P1[min(x + R, n - 1)] - P1[x - R - 1] + max(0, R - x) in[0] + max(0, x + R - (n - 1)) in[n - 1]: the clamped
//            overhang in closed form; <= 255 * 65535 < 2^24;
//   scan 2   of B1, in u64 (16384 * 255 * 65535 is about 2^46), kept as the segment-local inclusive prefix in u32 (a segment sums to
//            at most 64 * 2^24 = 2^30) in place plus the segment's u64 base: P2[i] = base[i >> SH] + local[i];
//   box 2    the same closed form on P2 with B1[0] and B1[n - 1], < 2^32, stored as the u32 row plane, coalesced.
// k_scatter_cols<T>: a wavefront owns kScatterStrip rows of 64 columns, a thread one column, so every access is a coalesced row
//   segment. With U the row plane and C[t] = sum_k U[clamp(t + k)] the first column box, a thread carries cA = C[clamp(y + R)],
//   cB = C[clamp(y - R)] and D = sum_j C[clamp(y + j)] in u64: D(y + 1) = D(y) + cA(y + 1) - cB(y), and a box moves from t to t + 1 by
//   U[clamp(t + 1 + R)] - U[clamp(t - R)] when 0 <= t < n - 1 and stays where the clamp holds it: four u32 loads an output, whether a
//   box moves is uniform over the wavefront (the loads are unconditional on clamped rows and the difference is masked, so that the
//   loads of the unrolled steps are in flight together). A strip starts by direct summation, 2R + 1 loads for cB and two more per step of the
//   2R steps to cA (763 at R = 127 against the 1024 of a strip's rows). The epilogue reads in[y, x], forms the mix and divides once
//   by the uniform d = b W, as a multiply-high: the numerator is below 2^16 d <= 2^16 * 64 * 255^4 < 2^54, and with l = max(10,
//   ceil(log2 d)) and m = floor(2^(54 + l) / d) + 1 < 2^64 (scatter_magic, on the host), 2^(54 + l) <= m d <= 2^(54 + l) + 2^l, so
//   floor(num m / 2^(54 + l)) = floor(num / d) for every num < 2^54 (Granlund and Montgomery 1994, theorem 4.2): the high 64 bits of
//   num m shifted right by l - 10. tests/test_scatter_division.py holds the inequality for every (R, b) and the quotients at the
//   multiples of d and just below them.
// Elements are read and written singly, so a plane needs no more than its element's alignment (image 1 of a batch with odd N^2 starts
// on a 2-byte boundary only). Nothing outside the three planes is read or written; they must not overlap.
#include "study_device.h"

namespace musica {

constexpr int kScatterThreads = 256;   // of a row workgroup
constexpr int kScatterStrip = 256;     // rows of a column wavefront
constexpr int kScatterCols = 64;       // its columns: one wavefront
static_assert(kScatterThreads << 6 >= 16384, "SH = 6 holds the largest side a context accepts");
static_assert(2 * ((kScatterThreads << 6) + kScatterThreads) * 4 + kScatterThreads * 8 + 64 <= 160 * 1024, "the LDS of a row workgroup at SH = 6");

template <typename T, int SH>
__global__ __launch_bounds__(kScatterThreads) void k_scatter_rows(const T* __restrict__ src, uint32_t* __restrict__ plane, int n, int R) {
    constexpr int kSeg = 1 << SH, kWords = (kScatterThreads << SH) + kScatterThreads;
    __shared__ uint32_t p1[kWords], p2[kWords];
    __shared__ unsigned long long base[kScatterThreads];
    __shared__ unsigned long long tot64[kScatterThreads / 64];
    __shared__ uint32_t tot32[kScatterThreads / 64];
    auto at = [](int i) { return i + (i >> SH); };
    const int tid = (int)threadIdx.x, s0 = tid << SH;
    src += (size_t)blockIdx.x * n;
    plane += (size_t)blockIdx.x * n;

    for (int i = tid; i < n; i += kScatterThreads) p1[at(i)] = src[i];
    __syncthreads();

    uint32_t run = 0;
    for (int k = 0; k < kSeg; k++)
        if (s0 + k < n) { run += p1[at(s0 + k)]; p1[at(s0 + k)] = run; }
    const uint32_t off1 = block_scan_exclusive(run, tot32);
    for (int k = 0; k < kSeg; k++)
        if (s0 + k < n) p1[at(s0 + k)] += off1;
    __syncthreads();

    const uint32_t in0 = p1[at(0)], in1 = n > 1 ? p1[at(n - 1)] - p1[at(n - 2)] : in0;
    for (int i = tid; i < n; i += kScatterThreads) {
        const int hi = min(i + R, n - 1), lo = i - R - 1;
        p2[at(i)] = p1[at(hi)] - (lo >= 0 ? p1[at(lo)] : 0u) + (uint32_t)max(0, R - i) * in0 + (uint32_t)max(0, i + R - (n - 1)) * in1;
    }
    __syncthreads();

    const unsigned long long b0 = p2[at(0)], b1 = p2[at(n - 1)];
    __syncthreads();                       // every thread has B1's ends before the scan overwrites them
    run = 0;
    for (int k = 0; k < kSeg; k++)
        if (s0 + k < n) { run += p2[at(s0 + k)]; p2[at(s0 + k)] = run; }
    base[tid] = block_scan_exclusive((unsigned long long)run, tot64);
    __syncthreads();

    for (int i = tid; i < n; i += kScatterThreads) {
        const int hi = min(i + R, n - 1), lo = i - R - 1;
        unsigned long long v = base[hi >> SH] + p2[at(hi)] + (unsigned long long)max(0, R - i) * b0 + (unsigned long long)max(0, i + R - (n - 1)) * b1;
        if (lo >= 0) v -= base[lo >> SH] + p2[at(lo)];
        plane[i] = (uint32_t)v;            // <= 255^2 * 65535 < 2^32
    }
}

template <typename T>
__global__ __launch_bounds__(kScatterCols) void k_scatter_cols(const uint32_t* __restrict__ plane, const T* __restrict__ src, T* __restrict__ out,
                                                                int n, int R, unsigned long long a, unsigned long long keep, unsigned long long half,
                                                                unsigned long long magic, int shift) {
    const int x = (int)blockIdx.x * kScatterCols + (int)threadIdx.x;
    const int y0 = (int)blockIdx.y * kScatterStrip, y1 = min(y0 + kScatterStrip, n);
    if (x >= n) return;
    const uint32_t* col = plane + x;
    auto u = [&](int y) { return (unsigned long long)col[(size_t)y * n]; };   // y in 0 .. n - 1
    // A box that the clamp holds in place adds nothing: the loads stay unconditional, on clamped rows, so that the unrolled steps'
    // loads are in flight together, and the difference is masked.
    auto moves = [](bool m) { return m ? ~0ull : 0ull; };

    // the strip's start: C[clamp(y0 - R)] directly, then the 2R steps to C[clamp(y0 + R)], every C on the way summed into D
    int t = y0 - R;
    const int tc = max(t, 0);
    unsigned long long c = 0;
    for (int k = -R; k <= R; k++) c += u(min(max(tc + k, 0), n - 1));
    const unsigned long long cb0 = c;
    unsigned long long d = c;
#pragma unroll 8
    for (int j = 1; j <= 2 * R; j++) {
        t++;
        c += (u(min(max(t + R, 0), n - 1)) - u(min(max(t - 1 - R, 0), n - 1))) & moves(t >= 1 && t <= n - 1);
        d += c;
    }
    unsigned long long ca = c, cb = cb0;

#pragma unroll 4
    for (int y = y0; y < y1; y++) {
        const size_t o = (size_t)y * n + x;
        out[o] = (T)(__umul64hi(keep * src[o] + a * d + half, magic) >> shift);
        ca += (u(min(y + 1 + 2 * R, n - 1)) - u(y)) & moves(y + R < n - 1);
        d += ca - cb;
        cb += (u(min(y + 1, n - 1)) - u(max(y - 2 * R, 0))) & moves(y - R >= 0);
    }
}

template <typename T, int SH>
static void launch_scatter_rows_as(hipStream_t st, const T* src, uint32_t* plane, int n, int radius) {
    hipLaunchKernelGGL((k_scatter_rows<T, SH>), dim3((unsigned)n), dim3(kScatterThreads), 0, st, src, plane, n, radius);
}

// The row launch with the smallest segment that holds a row of n.
template <typename T>
static void launch_scatter_rows(hipStream_t st, const T* src, uint32_t* plane, int n, int radius) {
    if (n <= kScatterThreads) launch_scatter_rows_as<T, 0>(st, src, plane, n, radius);
    else if (n <= kScatterThreads << 2) launch_scatter_rows_as<T, 2>(st, src, plane, n, radius);
    else if (n <= kScatterThreads << 4) launch_scatter_rows_as<T, 4>(st, src, plane, n, radius);
    else launch_scatter_rows_as<T, 6>(st, src, plane, n, radius);
}

// floor(num / d) = umul64hi(num, magic) >> shift for every num < 2^54 (k_scatter_cols' header); d = den (2 radius + 1)^4 >= 162.
struct ScatterMagic {
    unsigned long long magic;
    int shift;
};
static ScatterMagic scatter_magic(unsigned long long d) {
    int l = 10;
    while ((1ull << l) < d) l++;
    return {(unsigned long long)(((unsigned __int128)1 << (54 + l)) / d) + 1, l - 10};
}

template <typename T>
static void launch_scatter_cols(hipStream_t st, const uint32_t* plane, const T* src, T* out, int n, int radius, int num, int den) {
    const unsigned long long side = 2ull * (unsigned long long)radius + 1, w = side * side * side * side;
    const dim3 grid((unsigned)((n + kScatterCols - 1) / kScatterCols), (unsigned)((n + kScatterStrip - 1) / kScatterStrip));
    const unsigned long long d = (unsigned long long)den * w;
    const ScatterMagic g = scatter_magic(d);
    hipLaunchKernelGGL((k_scatter_cols<T>), grid, dim3(kScatterCols), 0, st, plane, src, out, n, radius, (unsigned long long)num,
                       (unsigned long long)(den - num) * w, d / 2, g.magic, g.shift);
}

template <typename T>
static void launch_scatter(hipStream_t st, const T* src, T* out, uint32_t* plane, int n, int radius, int num, int den) {
    launch_scatter_rows<T>(st, src, plane, n, radius);
    launch_scatter_cols<T>(st, plane, src, out, n, radius, num, den);
}

void launch_scatter_u16(hipStream_t st, const uint16_t* src, uint16_t* out, uint32_t* plane, int n, int radius, int num, int den) {
    launch_scatter<uint16_t>(st, src, out, plane, n, radius, num, den);
}
void launch_scatter_u8(hipStream_t st, const uint8_t* src, uint8_t* out, uint32_t* plane, int n, int radius, int num, int den) {
    launch_scatter<uint8_t>(st, src, out, plane, n, radius, num, den);
}

}  // namespace musica
