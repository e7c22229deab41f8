// kernels_expand_sd.hip — every launch of the pyramid that keeps a window of squares in registers, for gfx950 (CDNA4):
//
//   k_expand_fast<.., SD>  : the expand launches that compute the 5 x 5 RMS of their band image themselves (expand_march's SD branch,
//                            pyramid_march.h)                                                            launch_expand_sd
//   k_reduce_band_hist     : level 0's reduce + band march counting the level's noise histogram (reduce_band_block<true, true>,
//                            pyramid_march.h)                                                            launch_reduce_band_u16_hist
//   k_hist_seam            : the columns beside the strip boundaries that march leaves uncounted         launch_hist_seam
//   k_rb_sdev              : an sdev + noise-histogram pass (sdev_parts.h) or that seam, paired with the
//                            reduce + band march of the next level in one grid                           launch_rb_sdev
//
// A translation unit of its own because it is built with -fno-slp-vectorize (build.py NO_SLP): the window of six band rows of the SD
// expand launch takes 172 registers that way and 211 with the register pairs the SLP vectoriser builds for packed multiplies and adds,
// which on gfx950 cost what two plain ones cost (profiles/r04_valu_cost.txt). Every other pyramid launch is kernels_pyramid.hip's.
#include "pyramid_march.h"

namespace musica {

// Two launches that depend on the same producer and not on each other, as one: the sdev + noise-histogram pass of level i and reduce + band of
// level i + 1 both wait for reduce + band of level i only. Alone on the chip each is 1 - 2 wavefronts per SIMD of dependent arithmetic (8 x 2048^2:
// 45 us and 20 us at i = 0); as the two roles of one grid they fill each other's issue slots, and the pyramid's dependent chain RB1 -> RB2 -> RB3 -> RB4
// runs in the shadow of the sdev passes instead of in front of them. A role is a contiguous range of workgroups starting at a multiple of 8 (the XCD a
// workgroup runs on is its index % 8: the tile mapping of xcd_tile() holds inside a role, kernels_common.h role_tile).
// The seam of the level-0 march that counts its own noise histogram (reduce_band_block<true, true>): the two columns either side of every
// interior strip boundary, which that march leaves uncounted, from the stored band image. noise_hist.comp scans every (column, 16-row run)
// on its own (:20-47, m outer), so these runs are the shader's whatever launch counts them. One thread per column and run: 20 band rows x 5
// columns, vertical then horizontal sums of squares in sdev_values()' order, the literal sqrt(sum / 25) (what musica_rms25_8 returns),
// musica_noise_bin. Work item w of an image = (run, boundary, column): w % 4 = column 512 b - 2 + w % 4, so a boundary's four threads
// read one 32-byte piece of a row. `first`: the workgroup's first item; items: 4 x (strips - 1) x runs.
__device__ __forceinline__ void hist_seam_block(const float* __restrict__ band, int S, int pitch, uint32_t* __restrict__ hist, int cov,
                                                int first, int items, uint32_t* lh) {
    hist_lds_clear(lh);
    __syncthreads();
    const int w = first + (int)threadIdx.x;
    const int bounds = (S + kStripCols - 1) / kStripCols - 1;
    const int ci = w & 3, b = (w >> 2) % bounds + 1, run = (w >> 2) / bounds;
    const int x = b * kStripCols - 2 + ci, y0 = run * kHistArea;
    if (w < items && x < cov && y0 < cov) {   // columns and rows outside the dispatch coverage are not counted (cov is a multiple of 512)
        float q[kHistArea + 4][5];
#pragma unroll
        for (int r = 0; r < kHistArea + 4; r++) {
            const int y = y0 - 2 + r;
            const bool in = y >= 0 && y < S;
            const float* row = band + (size_t)(in ? y : 0) * pitch + (x - 2);   // columns x - 2 .. x + 2 lie inside the image: S >= 512 b + 8
#pragma unroll
            for (int m = 0; m < 5; m++) {
                const float v = in ? row[m] : 0.0f;   // rows outside the image read 0 (img_sdev.comp)
                q[r][m] = v * v;
            }
        }
        const uint32_t copy = (uint32_t)((threadIdx.x % kHistCopies) * kHistCopyStride);
        bool alive = true;
#pragma unroll
        for (int r = 0; r < kHistArea; r++) {
            float c[5];
#pragma unroll
            for (int m = 0; m < 5; m++) c[m] = sum5(q[r][m], q[r + 1][m], q[r + 2][m], q[r + 3][m], q[r + 4][m]);
            const float s = sqrtf(sum5(c[0], c[1], c[2], c[3], c[4]) / 25.0f);   // img_sdev.comp:30
            const int bin = musica_noise_bin(s);                                 // 0 = break (noise_hist.comp:29, :33, :39)
            alive = alive && bin != 0 && y0 + r < S;
            if (alive) atomicAdd(&lh[copy + (uint32_t)bin], 1u);                 // :45; bin 2048 is the pad word behind the copy (dropped, no break)
        }
    }
    __syncthreads();
    hist_lds_flush(lh, hist);
}
// the seam pass as a launch of its own (the scripts without pairs); grid: x = workgroups of an image, z = batch
__global__ __launch_bounds__(kBlockThreads) void k_hist_seam(const float* __restrict__ band, int S, int pitch, size_t plane, uint32_t* __restrict__ hist,
                                                             size_t hist_stride, int cov, int items) {
    __shared__ uint32_t lh[kHistLdsWords];
    const int img = (int)blockIdx.z;
    hist_seam_block(band + (size_t)img * plane, S, pitch, hist + (size_t)img * hist_stride, cov, (int)blockIdx.x * kBlockThreads, items, lh);
}
static inline int seam_items(int S, int cov) {
    const int bounds = (S + kStripCols - 1) / kStripCols - 1, rows = S < cov ? S : cov;
    return 4 * bounds * ((rows + kHistArea - 1) / kHistArea);
}
void launch_hist_seam(hipStream_t st, const float* band, const LevelDesc& l, uint32_t* hist, size_t hist_stride, int cov, int batch) {
    const int items = seam_items(l.S, cov);
    if (items <= 0) return;   // one strip: no seam
    hipLaunchKernelGGL(k_hist_seam, dim3((items + kBlockThreads - 1) / kBlockThreads, 1, batch), dim3(kBlockThreads), 0, st, band, l.S, l.pitch, l.plane,
                       hist, hist_stride, cov, items);
}

#ifndef MUSICA_RB_HIST_W
#define MUSICA_RB_HIST_W 2   // wavefronts per SIMD the register allocation is capped for
#endif
// Level 0's reduce + band launch counting the level's noise histogram itself (reduce_band_block<true, true>). Built here, without the SLP
// vectoriser, like the expand launches that keep a window of squares in registers.
__global__ __launch_bounds__(kBlockThreads, MUSICA_RB_HIST_W) void k_reduce_band_hist(const void* __restrict__ fine, float* __restrict__ down, float* __restrict__ band,
                                                               int S, int pitch, size_t plane, int Sc, int cpitch, size_t cplane,
                                                               int rows_per_wave, const uint32_t* __restrict__ minmax, int min_chain_exact,
                                                               uint16_t* __restrict__ le090, int swz, uint32_t* __restrict__ hist, size_t hist_stride, int cov) {
    __shared__ uint32_t lh[kHistLdsWords];
    hist_lds_clear(lh);
    __syncthreads();
    reduce_band_block<true, true>(fine, down, band, S, pitch, plane, Sc, cpitch, cplane, rows_per_wave, minmax, min_chain_exact, le090, xcd_tile(swz),
                                  (int)blockIdx.z, lh, cov);
    __syncthreads();
    hist_lds_flush(lh, hist + (size_t)blockIdx.z * hist_stride);
}
void launch_reduce_band_u16_hist(hipStream_t st, const uint16_t* px, float* down, float* band, const LevelDesc& lf, const LevelDesc& lc, int batch,
                                 int rows_per_wave, const uint32_t* minmax, int min_chain_exact, uint16_t* le090, int swz, uint32_t* hist,
                                 size_t hist_stride, int cov) {
    hipLaunchKernelGGL(k_reduce_band_hist, stream_grid(lf.S, lc.S, rows_per_wave, batch), dim3(kBlockThreads), 0, st, (const void*)px, down, band, lf.S,
                       lf.pitch, lf.plane, lc.S, lc.pitch, lc.plane, rows_per_wave, minmax, min_chain_exact, le090, swz, hist, hist_stride, cov);
}

__global__ __launch_bounds__(kBlockThreads, 4) void k_rb_sdev(const RbSdevArgs a) {
    __shared__ uint32_t lh[kHistLdsWords];
    __shared__ unsigned long long nzw[kWavesPerBlock][8];
    const int img = (int)blockIdx.z;
    Tile tile;
    if ((int)blockIdx.x >= a.rb_first) {   // block-uniform
        if (!role_tile((int)blockIdx.x - a.rb_first, a.rb_strips, a.rb_blocks, a.swz, tile)) return;
        reduce_band_block<false>(a.fine, a.down, a.band, a.S, a.pitch, a.plane, a.Sc, a.cpitch, a.cplane, a.rows_rb, nullptr, 0, nullptr, tile, img);
        return;
    }
    const SdevRunLevel& l = a.sl;
    if (l.rows < 0) {   // the level's march counted its own histogram: what is left of its pass is the seam (l.blocks workgroups)
        if ((int)blockIdx.x < l.blocks)
            hist_seam_block(l.band + (size_t)img * l.plane, l.S, l.pitch, l.hist + (size_t)img * a.hist_stride, a.cov, (int)blockIdx.x * kBlockThreads, a.seam_items, lh);
        return;
    }
    if (!role_tile((int)blockIdx.x, l.strips, l.blocks, a.swz, tile)) return;
    sdev_level_block<true, true, true>(l, tile, (size_t)img, a.hist_stride, a.cov, lh, nzw);
}
// `a`: the pointers, geometry of the reduce + band role and sl.{band, sdev, hist, rows} filled in by the caller; ls: the sdev level
void launch_rb_sdev(hipStream_t st, RbSdevArgs a, const LevelDesc& ls, int batch) {
    int s_strips = (ls.S + kStripCols - 1) / kStripCols;
    int s_blocks;
    a.seam_items = 0;
    if (a.sl.rows < 0) { a.seam_items = seam_items(ls.S, a.cov); s_strips = 1; s_blocks = (a.seam_items + kBlockThreads - 1) / kBlockThreads; }
    else s_blocks = sdev_blocks_per_strip(ls.S, a.sl.rows);
    a.sl.plane = ls.plane; a.sl.S = ls.S; a.sl.pitch = ls.pitch; a.sl.strips = s_strips; a.sl.blocks = s_blocks; a.sl.first = 0;
    a.rb_first = (s_strips * s_blocks + 7) & ~7;
    a.rb_strips = (a.S + kStripCols - 1) / kStripCols;
    const int segs = (a.Sc + a.rows_rb - 1) / a.rows_rb;
    a.rb_blocks = (segs + kWavesPerBlock - 1) / kWavesPerBlock;
    const int total = a.rb_first + ((a.rb_strips * a.rb_blocks + 7) & ~7);
    hipLaunchKernelGGL(k_rb_sdev, dim3(total, 1, batch), dim3(kBlockThreads), 0, st, a);
}

#ifndef MUSICA_SD_W
#define MUSICA_SD_W 3
#endif
#ifndef MUSICA_SD_CH_W
#define MUSICA_SD_CH_W 2   // with the CLAHE histogram on board the launch wants 189 registers: 64 bytes of scratch at 3 wavefronts per SIMD
#endif
// The expand launch of a level whose sdev image is not stored (a.sdev == nullptr; GAIN_CURVE levels 0 .. 2): kernels_pyramid.hip's
// launch_expand hands those over to this translation unit.
void launch_expand_sd(hipStream_t st, const ExpandArgs& a, bool nr, int batch) {
    const dim3 grid = stream_grid(a.S, a.Sc, a.rows_per_wave, batch);
    if (nr && a.ghist) {
        if (a.chist) hipLaunchKernelGGL((k_expand_fast<GAIN_CURVE, true, true, MUSICA_SD_CH_W, true, true>), grid, dim3(kBlockThreads), 0, st, a);
        else hipLaunchKernelGGL((k_expand_fast<GAIN_CURVE, true, true, MUSICA_SD_W, false, true>), grid, dim3(kBlockThreads), 0, st, a);
    }
    else if (nr) hipLaunchKernelGGL((k_expand_fast<GAIN_CURVE, true, false, MUSICA_SD_W, false, true>), grid, dim3(kBlockThreads), 0, st, a);
    else hipLaunchKernelGGL((k_expand_fast<GAIN_CURVE, false, false, MUSICA_SD_W, false, true>), grid, dim3(kBlockThreads), 0, st, a);
}

}  // namespace musica
