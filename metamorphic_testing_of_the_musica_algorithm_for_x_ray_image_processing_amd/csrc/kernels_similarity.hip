// kernels_similarity.hip — the metamorphic study's similarity metrics (harness.py: mse_similarity, ssim_similarity,
// hist_similarity; the reference's test/metamorphic_test/script.py:143-198) between the 8-bit output of a batch image and a stored
// 8-bit reference plane, on the device (musica_sim_compare, include/musica.h).
//
// Every query owns blockIdx.z. A workgroup of 256 threads owns a strip of 256 region columns, one column per thread, and marches down
// a segment of rows:
//   * side a is read as the graded f32 plane and quantised while it is loaded (out_u8: the pixels musica_get_out_pixels returns),
//     side b as the u8 plane of a reference slot;
//   * the sum of squared differences and the 256-entry value counts of both sides cover the pixels the workgroup owns (strip columns
//     0 .. 249, segment rows 0 .. R-1): each region pixel exactly once. Value counts go to LDS and are added to the query's counts with
//     one u32 atomic per non-zero bin at the end;
//   * SSIM: each thread keeps the vertical 7-row window sums of x, y, x^2, y^2 and xy of its column as int32 running sums (exact, so
//     nothing drifts), the 7 rows themselves in registers; the horizontal 7-sums come from an LDS row of the column sums. The window sums
//     of u8 data are integers, so they are exact; the per-pixel value is then harness.ssim_similarity's f64 expression in its order
//     (-ffp-contract=off, IEEE f64 division), and only the order of the final summation differs from numpy's. Strips overlap by the
//     6-column halo, segments by the 6-row halo.
// Per-workgroup SSIM and SSD partials are written to `part` and folded per query by k_sim_fold, both in study_device.h's fixed order:
// results are bit-identical from call to call (no f64 atomics).
#include <algorithm>

#include "study_device.h"

namespace musica {

constexpr int kSimThreads = kStudyThreads;
constexpr int kSimHalo = 3;                            // (7 - 1) / 2
constexpr int kSimCols = kSimThreads - 2 * kSimHalo;   // region columns a strip owns

// k_sim keeps its own reduction and SSIM text, not study_device.h's helpers: with them its median in devtools/sim_probe.py was 0.2 - 0.5 us
// of 87 slower in two A/B jobs (profiles/study_helpers_ab.txt). The order is the header's rule: wavefront tree, then the wavefronts in order.
__global__ __launch_bounds__(kSimThreads) void k_sim(const SimQueryDev* __restrict__ qs, SimPart* __restrict__ part, uint32_t* __restrict__ hist,
                                                     SimConsts k) {
    __shared__ uint32_t sh_a[256], sh_b[256];
    __shared__ uint4 row[2][kSimThreads];
    __shared__ double red_d[kSimThreads / 64];
    __shared__ unsigned long long red_u[kSimThreads / 64];
    const SimQueryDev q = qs[blockIdx.z];
    const int blk = blockIdx.x;
    if (blk >= q.strips * q.segs) return;   // whole workgroup: the grid is sized for the query with the most workgroups
    const int t = threadIdx.x;
    const int strip = blk % q.strips, seg = blk / q.strips;
    const int c = strip * kSimCols + t;                          // region column of this thread
    const bool col_in = c < q.w;
    const bool owns_col = t < kSimCols && col_in;
    const bool ssim_col = t >= kSimHalo && t < kSimThreads - kSimHalo && c < q.w - kSimHalo;
    const int r0 = seg * q.seg_rows;
    const int own_end = min(q.h, r0 + q.seg_rows);
    const int r1 = min(q.h, r0 + q.seg_rows + 2 * kSimHalo);     // rows loaded: the owned ones + the halo below
    sh_a[t] = 0u;
    sh_b[t] = 0u;
    __syncthreads();

    const float* __restrict__ pa = q.a + (col_in ? c : 0);
    const uint8_t* __restrict__ pb = q.b + (col_in ? c : 0);
    int32_t vx = 0, vy = 0, vxx = 0, vyy = 0, vxy = 0;   // vertical window sums of this column
    uint32_t rx[7] = {0, 0, 0, 0, 0, 0, 0}, ry[7] = {0, 0, 0, 0, 0, 0, 0};   // the window's rows (slot k: row j with (j - r0) % 7 == k)
    uint32_t ssd = 0u;    // <= 65025 * 16364 rows < 2^32
    double acc = 0.0;
    int p = 0;
    for (int j0 = r0; j0 < r1; j0 += 7) {
        uint32_t nx[7], ny[7];
#pragma unroll
        for (int kk = 0; kk < 7; kk++) {   // all loads of the group first: 14 in flight per thread
            const int j = j0 + kk;
            nx[kk] = 0u;
            ny[kk] = 0u;
            if (col_in && j < r1) {
                nx[kk] = out_u8(pa[(size_t)j * q.a_pitch]);
                ny[kk] = pb[(size_t)j * q.b_pitch];
            }
        }
#pragma unroll
        for (int kk = 0; kk < 7; kk++) {
            const int j = j0 + kk;
            if (j >= r1) break;   // uniform over the workgroup
            const int32_t x = (int32_t)nx[kk], y = (int32_t)ny[kk], ox = (int32_t)rx[kk], oy = (int32_t)ry[kk];
            rx[kk] = nx[kk];
            ry[kk] = ny[kk];
            vx += x - ox;
            vy += y - oy;
            vxx += x * x - ox * ox;
            vyy += y * y - oy * oy;
            vxy += x * y - ox * oy;
            if (owns_col && j < own_end) {
                const int32_t d = x - y;
                ssd += (uint32_t)(d * d);
                atomicAdd(&sh_a[x], 1u);
                atomicAdd(&sh_b[y], 1u);
            }
            if (j - r0 >= 2 * kSimHalo) {   // the window of centre row j - 3 is complete
                row[p][t] = make_uint4((uint32_t)vx | ((uint32_t)vy << 16), (uint32_t)vxx, (uint32_t)vyy, (uint32_t)vxy);
                __syncthreads();   // one barrier per row: the next row writes the other buffer
                if (ssim_col) {
                    uint4 s = row[p][t - 3];
#pragma unroll
                    for (int d = -2; d <= 3; d++) {
                        const uint4 v = row[p][t + d];
                        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;   // x | y << 16: both halves stay below 49 * 255 < 2^16
                    }
                    const double ux = (double)(s.x & 0xFFFFu) / 49.0, uy = (double)(s.x >> 16) / 49.0;
                    const double uxx = (double)s.y / 49.0, uyy = (double)s.z / 49.0, uxy = (double)s.w / 49.0;
                    const double vx_ = k.cov_norm * (uxx - ux * ux), vy_ = k.cov_norm * (uyy - uy * uy), vxy_ = k.cov_norm * (uxy - ux * uy);
                    acc += ((2.0 * ux * uy + k.c1) * (2.0 * vxy_ + k.c2)) / ((ux * ux + uy * uy + k.c1) * (vx_ + vy_ + k.c2));
                }
                p ^= 1;
            }
        }
    }
    // partials in a fixed order: wavefront tree, then the four wavefronts in order
    unsigned long long ssd64 = ssd;
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_down(acc, off, 64);
        ssd64 += __shfl_down(ssd64, off, 64);
    }
    if ((t & 63) == 0) {
        red_d[t >> 6] = acc;
        red_u[t >> 6] = ssd64;
    }
    __syncthreads();
    if (t == 0) {
        SimPart r;
        r.ssim = red_d[0];
        r.ssd = red_u[0];
        for (int w = 1; w < kSimThreads / 64; w++) {
            r.ssim += red_d[w];
            r.ssd += red_u[w];
        }
        part[(size_t)blockIdx.z * kSimMaxBlocks + blk] = r;
    }
    uint32_t* h = hist + (size_t)blockIdx.z * 512;
    if (sh_a[t]) atomicAdd(&h[t], sh_a[t]);
    if (sh_b[t]) atomicAdd(&h[256 + t], sh_b[t]);
}

// One workgroup per query: the partials of its workgroups in a fixed order.
__global__ __launch_bounds__(kSimThreads) void k_sim_fold(const SimQueryDev* __restrict__ qs, const SimPart* __restrict__ part, SimPart* __restrict__ out) {
    __shared__ WaveSlots<double> red_d;
    __shared__ WaveSlots<unsigned long long> red_u;
    const int t = threadIdx.x;
    const SimQueryDev q = qs[blockIdx.x];
    const int n = q.strips * q.segs;
    const SimPart* pp = part + (size_t)blockIdx.x * kSimMaxBlocks;
    double acc = 0.0;
    unsigned long long ssd = 0ull;
    for (int i = t; i < n; i += kSimThreads) {
        acc += pp[i].ssim;
        ssd += pp[i].ssd;
    }
    wave_sum(acc, ssd);
    if (wave_leader()) {
        red_d.put(acc);
        red_u.put(ssd);
    }
    __syncthreads();
    if (t == 0) out[blockIdx.x] = SimPart{red_d.sum(), red_u.sum()};
}

void strip_geometry(int w, int h, int cols, int cap, int& strips, int& segs, int& seg_rows) {
    strips = (w + cols - 1) / cols;
    const int want = std::max(1, cap / strips);
    const int n = std::max(1, std::min((h + 31) / 32, want));
    seg_rows = (h + n - 1) / n;
    segs = (h + seg_rows - 1) / seg_rows;
}

// a few hundred workgroups per query: enough to fill the chip for one comparison, few enough that the value-count flushes (up to 512
// same-address atomics per workgroup) stay short
void sim_geometry(SimQueryDev& q) { strip_geometry(q.w, q.h, kSimCols, std::min(kSimMaxBlocks, 512), q.strips, q.segs, q.seg_rows); }

void launch_sim(hipStream_t st, const SimQueryDev* d_qs, int count, int max_blocks, SimPart* part, uint32_t* hist, SimPart* out, const SimConsts& k) {
    hipLaunchKernelGGL(k_sim, dim3(max_blocks, 1, count), dim3(kSimThreads), 0, st, d_qs, part, hist, k);
    hipLaunchKernelGGL(k_sim_fold, dim3(count), dim3(kSimThreads), 0, st, d_qs, part, out);
}

// musica_sim_set_vendor_reference: the vendor-processed image into a reference slot, as the reference's script turns it into the 8-bit
// image it compares against (test/metamorphic_test/script.py:397-405: Image.point(i * 1/256).convert('L') for 16-bit data, then
// ImageOps.invert): 255 - (v >> 8) for u16, 255 - v for u8, truncating. Eight pixels per thread: 16 B (u16) or 8 B (u8) in, 8 B out,
// all aligned (both planes are dense from a hipMalloc base and a thread starts at a multiple of 8 pixels); the thread that holds the
// end of a plane whose size is not a multiple of 8 converts its tail one pixel at a time.
constexpr int kVendorThreads = 256;
constexpr int kVendorPx = 8;

// bytes 1 and 3 of a, then of b: the high bytes of four little-endian u16
__device__ __forceinline__ uint32_t high_bytes(uint32_t a, uint32_t b) {
    return ((a >> 8) & 0xFFu) | ((a >> 16) & 0xFF00u) | ((b << 8) & 0xFF0000u) | (b & 0xFF000000u);
}

template <typename T>
__global__ __launch_bounds__(kVendorThreads) void k_sim_vendor(const T* __restrict__ src, uint8_t* __restrict__ out, long long total) {
    const long long p0 = ((long long)blockIdx.x * kVendorThreads + threadIdx.x) * kVendorPx;
    if (p0 >= total) return;
    if (p0 + kVendorPx > total) {
        for (long long p = p0; p < total; p++) out[p] = (uint8_t)(255u - ((uint32_t)src[p] >> (8 * (sizeof(T) - 1))));
        return;
    }
    uint2 o;
    if constexpr (sizeof(T) == 2) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + p0);
        o = make_uint2(~high_bytes(v.x, v.y), ~high_bytes(v.z, v.w));   // ~b == 255 - b for every byte b
    } else {
        const uint2 v = *reinterpret_cast<const uint2*>(src + p0);
        o = make_uint2(~v.x, ~v.y);
    }
    *reinterpret_cast<uint2*>(out + p0) = o;
}

void launch_sim_vendor(hipStream_t st, const void* src, int bits, uint8_t* out, long long total) {
    const long long threads = (total + kVendorPx - 1) / kVendorPx;
    const unsigned blocks = (unsigned)((threads + kVendorThreads - 1) / kVendorThreads);
    if (bits == 16)
        hipLaunchKernelGGL(k_sim_vendor<uint16_t>, dim3(blocks), dim3(kVendorThreads), 0, st, static_cast<const uint16_t*>(src), out, total);
    else
        hipLaunchKernelGGL(k_sim_vendor<uint8_t>, dim3(blocks), dim3(kVendorThreads), 0, st, static_cast<const uint8_t*>(src), out, total);
}

}  // namespace musica
