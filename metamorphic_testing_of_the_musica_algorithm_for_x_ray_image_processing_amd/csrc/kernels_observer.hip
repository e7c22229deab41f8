// kernels_observer.hip — the model-observer relation of the study (include/musica.h, musica_sim_observer): the responses of square
// windows of an output and of a reference slot to banks of int8 templates, what a channelized Hotelling observer looks through. New,
// not in the reference. A view is (x, y, bank): an integer centre in the cropped output plane and the index of a bank
// {half, channels, weights[channels][S][S]}, S = 2 half + 1; its window |dx|, |dy| <= half lies inside the plane (the caller checks).
// Windows may overlap and views may repeat: the kernel only reads. Mathematically a gathered GEMM, [views x S^2] u8 . [S^2 x C] i8, in
// the study's integer idiom (v_dot4_u32_u8: dot4 of study_device.h), no float anywhere.
//
// k_observer: metrics.channel_responses. One workgroup of kStudyThreads per (view, block of kObserverBlock channels): grid.y is the
// block, and a block that starts at or behind the bank's channel count leaves at once. The host repacks a bank once per call
// (observer_pack) to [C][S][W] words, W = ceil(S / 4): four weights of a row a word, each BIASED to u8 (w + 128), the pad bytes of a
// row's last word 0. A row of the window is W pixel words the same way: side a is the graded f32 plane of a batch image quantised
// with out_u8 while it is read (load_quant4: exactly what k_sim reads), side b the slot's u8 plane (load_bytes4); both give zero bytes
// beyond the ragged tail (S is odd: every row has one), so a pad byte multiplies a zero and nothing outside the window is read. The
// S W words of the window are dealt to the threads round-robin, consecutive lanes on consecutive words of a row; a thread loads
// kObserverLoads of its words (pixels and weights) together, since the walk is bound by the latency of its loads. Per word a thread
// adds dot4(pixels, biased weights) into one u32 accumulator per channel of its block and side, and dot4(pixels, 0x01010101) into the
// side's plain sum, so that
//   R_j = sum a w_j = sum a (w_j + 128) - 128 sum a.
// The channel count is a runtime number: the accumulators are a register array of the compile-time block, and a channel behind the
// count reads the bank's last channel again and is written nowhere (an index into the array by a runtime number would spill it).
//   WIDTHS   the unsigned partials, of a thread as of the whole window: 255 * 255 * kObserverSide^2 = 255 * 255 * 17689
//            = 1 150 227 225 < 2^32, and 128 * 255 * 17689 = 577 368 960 < 2^31 bounds |R| (both asserted below): u32 accumulators are
//            exact, and the difference, taken modulo 2^32, is the exact int32.
// One integer workgroup reduction: wave_isum (DPP adds), the wavefronts' last lanes into WaveSlots, then thread k < kObserverBlock
// writes channel k's two responses and thread 0 of block 0 the two plain sums. No atomics: every word is written once, so the results
// repeat bit for bit. Traffic: per view and block S^2 5 B of pixels and (channels of the block) S W 4 B of weights, the weights from
// the cache after a bank's first view.
#include "study_device.h"

namespace musica {

constexpr int kObserverSide = 2 * kObserverMaxHalf + 1;
constexpr int kObserverLoads = 4;                       // window words of a thread whose loads are in flight together
constexpr int kObserverSums =2 * kObserverBlock + 2;   // the block's channels on side a, on side b, then the plain sums of a and b
static_assert(255ull * 255ull * kObserverSide * kObserverSide < (1ull << 32), "the unsigned partials over the largest window fit u32");
static_assert(255ull * 128ull * kObserverSide * kObserverSide < (1ull << 31), "a response over the largest window is an exact int32");
static_assert(kObserverMaxChannels % kObserverBlock == 0, "the blocks tile the largest channel count");

void observer_pack(const int8_t* weights, int half, int channels, std::vector<uint32_t>& words) {
    const int side = 2 * half + 1, row_words = (side + 3) / 4;
    const size_t first = words.size();
    words.resize(first + (size_t)channels * side * row_words, 0u);
    for (int j = 0; j < channels; j++)
        for (int row = 0; row < side; row++)
            for (int col = 0; col < side; col++) {
                const uint32_t biased = (uint32_t)((int)weights[((size_t)j * side + row) * side + col] + 128);
                words[first + ((size_t)j * side + row) * row_words + (col >> 2)] |= biased << (8 * (col & 3));
            }
}

// a: the graded f32 plane at output pixel (0, 0) (the margin skipped), b: the slot's plane; weights: observer_pack's words of every bank;
// tables: view i's 2 C int32 from its PackedView::table on; sums: count x 2 u32
__global__ __launch_bounds__(kStudyThreads) void k_observer(const float* __restrict__ a_plane, int a_pitch, const uint8_t* __restrict__ b_plane, int b_pitch,
                                                            const PackedView* __restrict__ views, const uint32_t* __restrict__ weights,
                                                            int32_t* __restrict__ tables, uint32_t* __restrict__ sums) {
    __shared__ WaveSlots<uint32_t, kObserverSums> slots;
    const PackedView v = views[blockIdx.x];   // uniform: the scalar side
    const int channels = (int)v.channels, j0 = (int)blockIdx.y * kObserverBlock;
    if (j0 >= channels) return;   // the whole workgroup alike, before any barrier
    const int half = (int)v.half, side = 2 * half + 1, row_words = (side + 3) >> 2, items = side * row_words;
    const GlobalF32* pa = (const GlobalF32*)a_plane + ((size_t)(v.y - half) * a_pitch + (v.x - half));
    const GlobalU8* pb = (const GlobalU8*)b_plane + ((size_t)(v.y - half) * b_pitch + (v.x - half));
    const GlobalU32* w = (const GlobalU32*)weights + v.weights;
    int chan[kObserverBlock];   // where each channel of the block starts in the bank's words
#pragma unroll
    for (int k = 0; k < kObserverBlock; k++) chan[k] = min(j0 + k, channels - 1) * items;

    uint32_t ra[kObserverBlock] = {}, rb[kObserverBlock] = {}, sa = 0u, sb = 0u;
    // kObserverLoads words of a thread at a time: their loads are issued together, or the walk would wait for one word after the
    // other (the largest window is 18 words a thread). A word past the window is the window's last word again, with zero pixels.
    for (int i0 = threadIdx.x; i0 < items; i0 += kObserverLoads * kStudyThreads) {
        uint32_t a[kObserverLoads], b[kObserverLoads], wk[kObserverLoads][kObserverBlock];
#pragma unroll
        for (int u = 0; u < kObserverLoads; u++) {
            const int i = min(i0 + u * kStudyThreads, items - 1);
            const int row = i / row_words, wd = i - row * row_words, col = wd << 2;
            a[u] = load_quant4(pa + (size_t)row * a_pitch + col, side - col);
            b[u] = load_bytes4(pb + (size_t)row * b_pitch + col, side - col);
#pragma unroll
            for (int k = 0; k < kObserverBlock; k++) wk[u][k] = w[chan[k] + i];
        }
#pragma unroll
        for (int u = 0; u < kObserverLoads; u++) {
            const bool live = i0 + u * kStudyThreads < items;
            const uint32_t va = live ? a[u] : 0u, vb = live ? b[u] : 0u;
            sa = dot4(va, 0x01010101u, sa);
            sb = dot4(vb, 0x01010101u, sb);
#pragma unroll
            for (int k = 0; k < kObserverBlock; k++) {
                ra[k] = dot4(va, wk[u][k], ra[k]);
                rb[k] = dot4(vb, wk[u][k], rb[k]);
            }
        }
    }
    // all 64 lanes are here again
    wave_isum(ra[0], ra[1], ra[2], ra[3], ra[4], ra[5], ra[6], ra[7], rb[0], rb[1], rb[2], rb[3], rb[4], rb[5], rb[6], rb[7], sa, sb);
    if (wave_last()) {   // the sums end in a wavefront's LAST lane; put() only looks at the wavefront's number
        uint32_t s[kObserverSums];
#pragma unroll
        for (int k = 0; k < kObserverBlock; k++) {
            s[k] = ra[k];
            s[kObserverBlock + k] = rb[k];
        }
        s[2 * kObserverBlock] = sa;
        s[2 * kObserverBlock + 1] = sb;
        slots.put(s);
    }
    __syncthreads();
    const int k = (int)threadIdx.x;
    if (k < kObserverBlock && j0 + k < channels) {
        int32_t* t = tables + v.table;
        t[j0 + k] = (int32_t)(slots.sum(k) - 128u * slots.sum(2 * kObserverBlock));                               // R_a
        t[channels + j0 + k] = (int32_t)(slots.sum(kObserverBlock + k) - 128u * slots.sum(2 * kObserverBlock + 1));   // R_b
    }
    if (k == 0 && blockIdx.y == 0) {
        sums[2 * blockIdx.x] = slots.sum(2 * kObserverBlock);
        sums[2 * blockIdx.x + 1] = slots.sum(2 * kObserverBlock + 1);
    }
}
static_assert(kObserverBlock == 8, "k_observer names its block's accumulators one by one for wave_isum");

void launch_sim_observer(hipStream_t st, const float* a_plane, int a_pitch, const uint8_t* b_plane, int b_pitch, const PackedView* d_views, int count,
                         int max_channels, const uint32_t* d_weights, int32_t* tables, uint32_t* sums) {
    const dim3 grid((unsigned)count, (unsigned)((max_channels + kObserverBlock - 1) / kObserverBlock));
    hipLaunchKernelGGL(k_observer, grid, dim3(kStudyThreads), 0, st, a_plane, a_pitch, b_plane, b_pitch, d_views, d_weights, tables, sums);
}

}  // namespace musica
