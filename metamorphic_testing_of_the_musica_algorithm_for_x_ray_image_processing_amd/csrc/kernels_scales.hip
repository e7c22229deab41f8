// kernels_scales.hip — scale-resolved SSIM of the study (musica_sim_multiscale, include/musica.h; harness.py multiscale_similarities):
// the 7 x 7 SSIM, its contrast-structure and luminance factors and the squared difference of a comparison at scales 0 .. scales - 1,
// scale s being the planes of 2^s x 2^s block SUMS of both sides (iterated 2 x 2 mean pooling times 4^s: integers, so every window sum
// at every scale is exact). Side a is the graded f32 plane of a batch image quantised with out_u8 while it is read, exactly what k_sim
// compares; side b a reference slot.
//
// k_scales_pool: the only pass over the full-resolution planes. A query owns blockIdx.z, a workgroup of 256 threads a tile of 64 x 16
// region pixels anchored at the region's origin (so its 16 x 16 blocks are the blocks of every scale): thread t loads column t % 64 of
// rows 4 (t / 64) .. + 3, 256 contiguous bytes of a per wavefront and row. Pixels outside the region are 0 and never loaded.
//   * Scale 0 goes to the call's scratch as x | y << 8 (u16 per pixel).
//   * x | y << 16 of a pixel is one u32 whose halves add without carrying into each other up to scale 4 (255 * 4^4 = 65280 < 2^16), so a
//     block sum of both sides is one integer add per level: vertical pairs in registers, then four levels through LDS (64 x 8 pair sums
//     -> 32 x 8 -> 16 x 4 -> 8 x 2 -> 4 x 1 cells). A cell is stored (u32 per texel, x in the low half) and counted only when its block
//     lies inside the region: plane s is (h >> s) x (w >> s), rows and columns that do not fill a block are dropped.
//   * (X - Y)^2 of every stored cell (and of every region pixel at scale 0) is summed per thread in u64, reduced over the workgroup and
//     written as the tile's partial: integers, exact in any order.
// k_scales_win: one launch over all queries x scales, a job (query, scale) per blockIdx.y. k_sim's march over the job's plane: a
// workgroup owns a strip of 256 plane columns, one per thread, and a segment of rows; each thread keeps the vertical 7-row window sums of
// x, y, x^2, y^2 and xy of its column as running integer sums, the 7 rows themselves in registers (so nothing drifts), and the
// horizontal 7-sums come from an LDS row of the column sums. u32 sums for scales 0 .. 2 (49 * (255 * 16)^2 < 2^32), u64 from scale 3 on
// (49 * (255 * 256)^2 = 2.09e11); arithmetic mod 2^32 / 2^64 on values that fit is exact. The per-window value is then
// harness.multiscale_similarities' f64 expression in its order (-ffp-contract=off, IEEE f64 division): one division per mean by the
// exact doubles 49 * 4^s and 49 * 16^s, then ssim_similarity's terms. Three f64 accumulators per thread (ssim, cs, lum).
// Per-workgroup partials are folded per job by k_scales_fold (with the tiles' integer partials), both in study_device.h's fixed order:
// no f64 atomics, results are bit-identical from call to call.
#include <algorithm>

#include "study_device.h"

namespace musica {

constexpr int kScaleThreads = kStudyThreads;
constexpr int kScaleHalo = 3;                              // (7 - 1) / 2
constexpr int kScaleCols = kScaleThreads - 2 * kScaleHalo; // plane columns a strip owns

__device__ __forceinline__ unsigned long long sq_diff_packed(uint32_t p) {   // (x - y)^2 of x | y << 16
    const long long d = (long long)(p & 0xFFFFu) - (long long)(p >> 16);
    return (unsigned long long)(d * d);
}

__global__ __launch_bounds__(kScaleThreads) void k_scales_pool(const ScalePoolDev* __restrict__ qs, uint8_t* __restrict__ scratch,
                                                               ScalePoolPart* __restrict__ part) {
    __shared__ uint32_t l0[8][kScalePoolW];            // vertical pair sums of the tile's columns
    __shared__ uint32_t l1[8][kScalePoolW / 2];        // scale-1 cells
    __shared__ uint32_t l2[4][kScalePoolW / 4];
    __shared__ uint32_t l3[2][kScalePoolW / 8];
    __shared__ WaveSlots<unsigned long long, kScaleMaxScales> red;
    const ScalePoolDev q = qs[blockIdx.z];
    const int blk = blockIdx.x;
    if (blk >= q.tiles_x * q.tiles_y) return;   // whole workgroup: the grid is sized for the query with the most tiles
    const int t = threadIdx.x;
    const int tx = blk % q.tiles_x, ty = blk / q.tiles_x;
    unsigned long long ssd[kScaleMaxScales] = {0ull, 0ull, 0ull, 0ull, 0ull};

    {   // scale 0: load, quantise, store, vertical pairs
        const int lc = t & (kScalePoolW - 1), g = t >> 6;
        const int c = tx * kScalePoolW + lc;
        uint16_t* __restrict__ p0 = reinterpret_cast<uint16_t*>(scratch + q.plane_off[0]);
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int r = ty * kScalePoolH + 4 * g + k;
            p[k] = 0u;
            if (c < q.w && r < q.h) {
                const uint32_t x = out_u8(q.a[(size_t)r * q.a_pitch + c]), y = q.b[(size_t)r * q.b_pitch + c];
                p[k] = x | (y << 16);
                p0[(size_t)r * q.w + c] = (uint16_t)(x | (y << 8));
                ssd[0] += sq_diff_packed(p[k]);
            }
        }
        l0[2 * g][lc] = p[0] + p[1];
        l0[2 * g + 1][lc] = p[2] + p[3];
    }
    __syncthreads();
    if (q.scales > 1) {   // uniform over the workgroup, as every test of q.scales below
        const int r = t >> 5, c = t & 31;
        const uint32_t v = l0[r][2 * c] + l0[r][2 * c + 1];
        l1[r][c] = v;
        const int pr = ty * (kScalePoolH >> 1) + r, pc = tx * (kScalePoolW >> 1) + c, pw = q.w >> 1;
        if (pr < (q.h >> 1) && pc < pw) {
            reinterpret_cast<uint32_t*>(scratch + q.plane_off[1])[(size_t)pr * pw + pc] = v;
            ssd[1] += sq_diff_packed(v);
        }
    }
    __syncthreads();
    if (q.scales > 2 && t < 64) {
        const int r = t >> 4, c = t & 15;
        const uint32_t v = l1[2 * r][2 * c] + l1[2 * r][2 * c + 1] + l1[2 * r + 1][2 * c] + l1[2 * r + 1][2 * c + 1];
        l2[r][c] = v;
        const int pr = ty * (kScalePoolH >> 2) + r, pc = tx * (kScalePoolW >> 2) + c, pw = q.w >> 2;
        if (pr < (q.h >> 2) && pc < pw) {
            reinterpret_cast<uint32_t*>(scratch + q.plane_off[2])[(size_t)pr * pw + pc] = v;
            ssd[2] += sq_diff_packed(v);
        }
    }
    __syncthreads();
    if (q.scales > 3 && t < 16) {
        const int r = t >> 3, c = t & 7;
        const uint32_t v = l2[2 * r][2 * c] + l2[2 * r][2 * c + 1] + l2[2 * r + 1][2 * c] + l2[2 * r + 1][2 * c + 1];
        l3[r][c] = v;
        const int pr = ty * (kScalePoolH >> 3) + r, pc = tx * (kScalePoolW >> 3) + c, pw = q.w >> 3;
        if (pr < (q.h >> 3) && pc < pw) {
            reinterpret_cast<uint32_t*>(scratch + q.plane_off[3])[(size_t)pr * pw + pc] = v;
            ssd[3] += sq_diff_packed(v);
        }
    }
    __syncthreads();
    if (q.scales > 4 && t < 4) {
        const uint32_t v = l3[0][2 * t] + l3[0][2 * t + 1] + l3[1][2 * t] + l3[1][2 * t + 1];
        const int pr = ty, pc = tx * (kScalePoolW >> 4) + t, pw = q.w >> 4;
        if (pr < (q.h >> 4) && pc < pw) {
            reinterpret_cast<uint32_t*>(scratch + q.plane_off[4])[(size_t)pr * pw + pc] = v;
            ssd[4] += sq_diff_packed(v);
        }
    }
    // the tile's partial: thread s folds scale s
#pragma unroll
    for (int s = 0; s < kScaleMaxScales; s++) wave_sum(ssd[s]);
    if (wave_leader()) red.put(ssd);
    __syncthreads();
    if (t < kScaleMaxScales) part[q.part_base + blk].ssd[t] = red.sum(t);
}

// The march of one job. T: the window sums' integer type; TEXEL: u16 (x | y << 8, scale 0) or u32 (x | y << 16).
template <typename T, typename TEXEL>
__device__ __forceinline__ void scales_march(const ScaleJobDev& q, const uint8_t* __restrict__ scratch, T* __restrict__ row /* [2][5][256] */,
                                             const ScaleConsts& k, int blk, double& a_ssim, double& a_cs, double& a_lum) {
    constexpr int kShift = sizeof(TEXEL) == 2 ? 8 : 16;
    constexpr uint32_t kMask = (1u << kShift) - 1u;
    const int t = threadIdx.x;
    const int strip = blk % q.strips, seg = blk / q.strips;
    const int c = strip * kScaleCols + t;                        // plane column of this thread
    const bool col_in = c < q.w;
    const bool win_col = t >= kScaleHalo && t < kScaleThreads - kScaleHalo && c < q.w - kScaleHalo;
    const int r0 = seg * q.seg_rows;
    const int r1 = min(q.h, r0 + q.seg_rows + 2 * kScaleHalo);   // rows loaded: the segment's + the halo below
    const TEXEL* __restrict__ pp = reinterpret_cast<const TEXEL*>(scratch + q.plane_off) + (col_in ? c : 0);
    const double d1 = k.div1[q.scale], d2 = k.div2[q.scale];
    T vx = 0, vy = 0, vxx = 0, vyy = 0, vxy = 0;                 // vertical window sums of this column (mod 2^bits: exact)
    uint32_t rr[7] = {0, 0, 0, 0, 0, 0, 0};                      // the window's rows (slot kk: row j with (j - r0) % 7 == kk), as loaded
    int p = 0;
    for (int j0 = r0; j0 < r1; j0 += 7) {
        uint32_t nn[7];
#pragma unroll
        for (int kk = 0; kk < 7; kk++) {   // all loads of the group first
            const int j = j0 + kk;
            nn[kk] = 0u;
            if (col_in && j < r1) nn[kk] = pp[(size_t)j * q.w];
        }
#pragma unroll
        for (int kk = 0; kk < 7; kk++) {
            const int j = j0 + kk;
            if (j >= r1) break;   // uniform over the workgroup
            const uint32_t x = nn[kk] & kMask, y = nn[kk] >> kShift, ox = rr[kk] & kMask, oy = rr[kk] >> kShift;   // <= 65280: products fit u32
            rr[kk] = nn[kk];
            vx += (T)x - (T)ox;
            vy += (T)y - (T)oy;
            vxx += (T)(x * x) - (T)(ox * ox);
            vyy += (T)(y * y) - (T)(oy * oy);
            vxy += (T)(x * y) - (T)(ox * oy);
            if (j - r0 >= 2 * kScaleHalo) {   // the window of centre row j - 3 is complete
                T* __restrict__ rw = row + p * 5 * kScaleThreads;
                rw[t] = vx;
                rw[kScaleThreads + t] = vy;
                rw[2 * kScaleThreads + t] = vxx;
                rw[3 * kScaleThreads + t] = vyy;
                rw[4 * kScaleThreads + t] = vxy;
                __syncthreads();   // one barrier per row: the next row writes the other buffer
                if (win_col) {
                    T s[5];
#pragma unroll
                    for (int f = 0; f < 5; f++) {
                        T v = rw[f * kScaleThreads + t - 3];
#pragma unroll
                        for (int d = -2; d <= 3; d++) v += rw[f * kScaleThreads + t + d];
                        s[f] = v;
                    }
                    const double ux = (double)s[0] / d1, uy = (double)s[1] / d1;
                    const double uxx = (double)s[2] / d2, uyy = (double)s[3] / d2, uxy = (double)s[4] / d2;
                    const SsimTerms m = ssim_terms(ux, uy, uxx, uyy, uxy, k);
                    a_ssim += (m.a1 * m.a2) / (m.b1 * m.b2);
                    a_cs += m.a2 / m.b2;
                    a_lum += m.a1 / m.b1;
                }
                p ^= 1;
            }
        }
    }
}

__global__ __launch_bounds__(kScaleThreads) void k_scales_win(const ScaleJobDev* __restrict__ jobs, const uint8_t* __restrict__ scratch,
                                                              ScaleWinPart* __restrict__ part, ScaleConsts k) {
    __shared__ unsigned long long row[2 * 5 * kScaleThreads];
    __shared__ WaveSlots<double, 3> red;
    const ScaleJobDev q = jobs[blockIdx.y];
    const int blk = blockIdx.x;
    if (blk >= q.strips * q.segs) return;   // whole workgroup: the grid is sized for the job with the most workgroups
    double acc[3] = {0.0, 0.0, 0.0};
    if (q.scale == 0) scales_march<uint32_t, uint16_t>(q, scratch, reinterpret_cast<uint32_t*>(row), k, blk, acc[0], acc[1], acc[2]);
    else if (q.scale <= 2) scales_march<uint32_t, uint32_t>(q, scratch, reinterpret_cast<uint32_t*>(row), k, blk, acc[0], acc[1], acc[2]);
    else scales_march<unsigned long long, uint32_t>(q, scratch, row, k, blk, acc[0], acc[1], acc[2]);
#pragma unroll
    for (int f = 0; f < 3; f++) wave_sum(acc[f]);
    if (wave_leader()) red.put(acc);
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * kScaleMaxBlocks + blk] = ScaleWinPart{red.sum(0), red.sum(1), red.sum(2)};
}

// One workgroup per job: the partials of its workgroups, and its scale's integer partials of its query's tiles, in a fixed order.
__global__ __launch_bounds__(kScaleThreads) void k_scales_fold(const ScaleJobDev* __restrict__ jobs, const ScalePoolDev* __restrict__ qs,
                                                               const ScaleWinPart* __restrict__ part, const ScalePoolPart* __restrict__ pool,
                                                               ScaleOut* __restrict__ out) {
    __shared__ WaveSlots<double, 3> red_d;
    __shared__ WaveSlots<unsigned long long> red_u;
    const int t = threadIdx.x;
    const ScaleJobDev q = jobs[blockIdx.x];
    const ScalePoolDev pq = qs[q.query];
    const int n = q.strips * q.segs, tiles = pq.tiles_x * pq.tiles_y;
    const ScaleWinPart* pp = part + (size_t)blockIdx.x * kScaleMaxBlocks;
    double acc[3] = {0.0, 0.0, 0.0};
    unsigned long long ssd = 0ull;
    for (int i = t; i < n; i += kScaleThreads) {
        acc[0] += pp[i].ssim;
        acc[1] += pp[i].cs;
        acc[2] += pp[i].lum;
    }
    for (int i = t; i < tiles; i += kScaleThreads) ssd += pool[pq.part_base + i].ssd[q.scale];
    wave_sum(acc[0], acc[1], acc[2], ssd);
    if (wave_leader()) {
        red_d.put(acc);
        red_u.put(ssd);
    }
    __syncthreads();
    if (t == 0) out[blockIdx.x] = ScaleOut{red_d.sum(0), red_d.sum(1), red_d.sum(2), red_u.sum()};
}

void scales_geometry(ScaleJobDev& q) { strip_geometry(q.w, q.h, kScaleCols, kScaleMaxBlocks, q.strips, q.segs, q.seg_rows); }

void launch_scales(hipStream_t st, const ScalePoolDev* d_qs, int count, int max_tiles, const ScaleJobDev* d_jobs, int jobs, int max_blocks,
                   uint8_t* scratch, ScalePoolPart* pool, ScaleWinPart* part, ScaleOut* out, const ScaleConsts& k) {
    hipLaunchKernelGGL(k_scales_pool, dim3(max_tiles, 1, count), dim3(kScaleThreads), 0, st, d_qs, scratch, pool);
    hipLaunchKernelGGL(k_scales_win, dim3(max_blocks, jobs), dim3(kScaleThreads), 0, st, d_jobs, scratch, part, k);
    hipLaunchKernelGGL(k_scales_fold, dim3(jobs), dim3(kScaleThreads), 0, st, d_jobs, d_qs, part, pool, out);
}

}  // namespace musica
