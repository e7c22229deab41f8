// kernels_gradients.hip — the gradient metrics of the study (musica_sim_gradients, include/musica.h; metrics.gradient_statistics): the
// integer Sobel gradients of both sides of a comparison over the interior of its region, their exact sums kept apart by the edge
// strength of the REFERENCE side, and the mean of a per-pixel gradient similarity. Side a is the graded f32 plane of a batch image
// quantised with out_u8 while it is read (load_quant4: exactly what k_sim reads), side b a reference slot.
//
// k_gradients: a query owns blockIdx.z, a workgroup of kStudyThreads threads one 64 x 64 tile of the query's INTERIOR, the (w - 2) x
// (h - 2) pixels whose 3 x 3 neighbourhood lies inside the region (tile_geom over the interior).
//   stage    the (tw + 2) x (th + 2) windows of both sides, at most 66 x 66, once, as packed bytes in LDS (stage_windows): 4 + 1 bytes
//            per window pixel, nothing outside the region is read.
//   columns  a thread takes four neighbouring pixels of a row, sixteen lanes a tile row, four rows a wavefront, four trips a tile. It
//            reads two words of each of the three window rows, forms the column sums t + 2 m + b and differences b - t of its six
//            columns ONCE, and the four gx = s[i + 2] - s[i], gy = d[i] + 2 d[i + 1] + d[i + 2] from them.
//   terms    A = gxa^2 + gya^2, B = gxb^2 + gyb^2, dot, cross: |term| <= kGradMaxTerm. The class is the bit length of B, 32 - clz(B).
//   q        (2 dot + C) / (A + B + C), exact integers below 2^53 and one IEEE f64 division; a thread adds its sixteen q in trip and
//            pixel order, then study_device.h's ONE order over the workgroup; the tile's partial is stored, never added atomically.
// THE ACCUMULATION. A real output puts most pixels into three or four classes and a flat reference all of them into class 0, so
// per-pixel LDS atomics would serialise on a handful of addresses. There are none. Per trip a wavefront walks the classes 0 .. 21 and
// skips, with one ballot each, those that none of its 256 pixels has; for a class that is present every lane sums the terms of its
// pixels of that class (0 .. 4 of them), the five words n | neg << 16, A, B, dot, cross go through ONE wave_isum (integers: DPP adds,
// no ds_bpermute), and the wavefront's last lane adds them, with plain LDS adds, into the wavefront's OWN [22][5] table of 32-bit
// words. A flat reference costs one reduction a trip, random bytes the four or five classes they reach.
// THE 32-BIT RULE. A wavefront counts at most kGradWavePixels = 16 rows x 64 columns = 1024 pixels of a tile, so a word of its table is at
// most 1024 x 1 300 500 = 1 331 712 000 < 2^31 in magnitude (32 bits hold 3302 pixels' worth, signed 1651: asserted below), n and neg at
// most 1024 < 2^16. A tile's sum does not fit (4096 x 1 300 500 > 2^32; vertical stripes of period 4 reach 4096 x 1 040 400 > 2^31, more
// than a signed word, in sum dot): the four tables are widened to 64 bits, dot and cross sign-extended, where they are combined, one
// table word a thread, and the non-zero words are added to the query's table with 64-bit integer global atomics (the caller zeroes
// the tables on the stream). Integer sums commute: exact and identical from call to call.
// k_gradients_fold: one workgroup a query, the tiles' q partials in study_device.h's order.
#include "study_device.h"

namespace musica {

constexpr int kGradWinWords = (kSimTile + 2 + 3) / 4;          // words of a staged window row: 66 pixels
constexpr int kGradWinRows = kSimTile + 2;
constexpr int kGradLanes = kSimTile / 4;                       // lanes of a tile row, four pixels each
constexpr int kGradRows = kStudyThreads / kGradLanes;          // tile rows of a trip
constexpr int kGradTrips = kSimTile / kGradRows;
constexpr int kGradWavePixels = kSimTile * kSimTile / kStudyWaves;   // what a wavefront counts of a tile
constexpr int kGradWaveWords = 5;                              // n | neg << 16, A, B, dot, cross
constexpr long long kGradMaxTerm = 1300500;                    // 1020^2 + 510^2, the neighbourhood [[0,0,255],[0,.,255],[0,255,255]]
static_assert(kGradWinWords == 17 && kGradLanes == 16 && kGradRows == 16 && kGradTrips == 4, "16 lanes a row, 4 rows a wavefront, 4 trips a tile; a thread's two words end at word 16");
static_assert(kGradWavePixels == 1024 && kGradWavePixels * kGradMaxTerm < (1ll << 31) && kGradWavePixels < (1 << 16),
              "THE 32-BIT RULE: a wavefront's share of a tile fits a signed 32-bit word, its counts 16 bits");
static_assert(kGradClasses == 22 && (kGradMaxTerm >> (kGradClasses - 1)) == 0 && (kGradMaxTerm >> (kGradClasses - 2)) == 1, "the bit length of B is at most 21, and 21 is reached");
static_assert(kGradClasses * kGradWords <= kStudyThreads, "one table word a thread");

// The column sums t + 2 m + b and differences b - t of the six columns from byte 0 of word `wd` of window rows r .. r + 2
__device__ __forceinline__ void grad_columns(const uint32_t* __restrict__ win, int r, int wd, int (&s)[6], int (&d)[6]) {
    const uint32_t* p = win + r * kGradWinWords + wd;
    const uint32_t t[2] = {p[0], p[1]}, m[2] = {p[kGradWinWords], p[kGradWinWords + 1]}, b[2] = {p[2 * kGradWinWords], p[2 * kGradWinWords + 1]};
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const int sh = 8 * (c & 3);
        const int tt = (int)((t[c >> 2] >> sh) & 0xFFu), mm = (int)((m[c >> 2] >> sh) & 0xFFu), bb = (int)((b[c >> 2] >> sh) & 0xFFu);
        s[c] = tt + 2 * mm + bb;
        d[c] = bb - tt;
    }
}

__global__ __launch_bounds__(kStudyThreads) void k_gradients(const GradQueryDev* __restrict__ qs, unsigned long long* __restrict__ tables, double* __restrict__ part) {
    __shared__ uint32_t wa[kGradWinRows * kGradWinWords], wb[kGradWinRows * kGradWinWords];
    __shared__ uint32_t tab[kStudyWaves][kGradClasses][kGradWaveWords];
    __shared__ WaveSlots<double> red;
    const GradQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.tiles_x * q.tiles_y) return;   // whole workgroup: the grid is sized for the query with the most tiles
    const TileGeom g = tile_geom(blockIdx.x, q.tiles_x, q.w - 2, q.h - 2);   // of the interior: window pixel (0, 0) is region pixel (x0, y0)
    const int t = threadIdx.x;
    for (int i = t; i < kStudyWaves * kGradClasses * kGradWaveWords; i += kStudyThreads) (&tab[0][0][0])[i] = 0u;
    stage_windows((const GlobalF32*)q.a + (ptrdiff_t)g.y0 * q.a_pitch + g.x0, q.a_pitch, (const GlobalU8*)q.b + (ptrdiff_t)g.y0 * q.b_pitch + g.x0, q.b_pitch,
                  g.tw + 2, g.th + 2, wa, wb, kGradWinWords, kGradWinWords, kGradWinRows);
    __syncthreads();

    const int lane = t & (kGradLanes - 1), cx = lane * 4, r = t / kGradLanes;
    uint32_t* __restrict__ mine = &tab[t >> 6][0][0];
    double acc = 0.0;
    for (int k = 0; k < kGradTrips; k++) {
        const int ty = k * kGradRows + r;
        int sa[6], da[6], sb[6], db[6];
        grad_columns(wa, ty, lane, sa, da);   // rows ty .. ty + 2 <= 65, words lane, lane + 1 <= 16: inside the staged window
        grad_columns(wb, ty, lane, sb, db);
        uint32_t A[4], B[4], present = 0u;
        int dot[4], cross[4], cls[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int gxa = sa[i + 2] - sa[i], gya = da[i] + 2 * da[i + 1] + da[i + 2];
            const int gxb = sb[i + 2] - sb[i], gyb = db[i] + 2 * db[i + 1] + db[i + 2];
            A[i] = (uint32_t)(gxa * gxa + gya * gya);
            B[i] = (uint32_t)(gxb * gxb + gyb * gyb);
            dot[i] = gxa * gxb + gya * gyb;
            cross[i] = gxa * gyb - gya * gxb;
            const bool in = ty < g.th && cx + i < g.tw;
            cls[i] = in ? 32 - __clz((int)B[i]) : -1;
            if (in) {
                present |= 1u << cls[i];
                acc += (double)(2 * dot[i] + kGradC) / (double)(A[i] + B[i] + (uint32_t)kGradC);
            }
        }
        for (int c = 0; c < kGradClasses; c++) {
            if (__ballot((present >> c) & 1u) == 0ull) continue;   // uniform over the wavefront
            uint32_t n = 0u, a = 0u, b = 0u;
            int dd = 0, cc = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (cls[i] != c) continue;
                n += 1u + (dot[i] < 0 ? 0x10000u : 0u);
                a += A[i];
                b += B[i];
                dd += dot[i];
                cc += cross[i];
            }
            wave_isum(n, a, b, dd, cc);   // at most 256 pixels: every word below 2^29; all 64 lanes are here (the ballot is uniform)
            if (wave_last()) {
                uint32_t* row = mine + c * kGradWaveWords;
                row[0] += n;
                row[1] += a;
                row[2] += b;
                row[3] += (uint32_t)dd;
                row[4] += (uint32_t)cc;
            }
        }
    }
    wave_sum(acc);
    if (wave_leader()) red.put(acc);
    __syncthreads();
    if (t == 0) part[q.tile_base + blockIdx.x] = red.sum();
    if (t < kGradClasses * kGradWords) {   // word f of class c, the four wavefronts widened to 64 bits
        const int c = t / kGradWords, f = t - c * kGradWords;
        unsigned long long v = 0ull;
        for (int w = 0; w < kStudyWaves; w++) {
            const uint32_t* row = tab[w][c];
            v += f == 0   ? (unsigned long long)(row[0] & 0xFFFFu)
                 : f == 5 ? (unsigned long long)(row[0] >> 16)
                 : f <= 2 ? (unsigned long long)row[f]
                          : (unsigned long long)(long long)(int32_t)row[f];
        }
        if (v) atomicAdd((unsigned long long*)((GlobalU64*)tables + q.table + (size_t)c * kGradWords + f), v);
    }
}

// One workgroup per query: the partials of its tiles in a fixed order
__global__ __launch_bounds__(kStudyThreads) void k_gradients_fold(const GradQueryDev* __restrict__ qs, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ WaveSlots<double> red;
    const GradQueryDev q = qs[blockIdx.x];
    const int n = q.tiles_x * q.tiles_y;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += kStudyThreads) acc += part[q.tile_base + i];
    wave_sum(acc);
    if (wave_leader()) red.put(acc);
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = red.sum();
}

void launch_sim_gradients(hipStream_t st, const GradQueryDev* d_qs, int count, int max_tiles, unsigned long long* tables, double* part, double* out) {
    hipLaunchKernelGGL(k_gradients, dim3((unsigned)max_tiles, 1, (unsigned)count), dim3(kStudyThreads), 0, st, d_qs, tables, part);
    hipLaunchKernelGGL(k_gradients_fold, dim3((unsigned)count), dim3(kStudyThreads), 0, st, d_qs, part, out);
}

}  // namespace musica
