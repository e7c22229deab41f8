// kernels_pyramid.hip — the Laplacian-pyramid kernels of the MUSICA path for gfx950 (CDNA4).
//
//   k_reduce_*  : img_smooth.comp + img_downsample.comp fused            (K5 + K6, the metric kernel)
//   k_band_*    : img_upsample.comp + img_smooth_upsampled.comp + img_difference.comp fused (K7 + K8 + K9)
//   k_expand_*  : contrast_curve_apply.comp + noise_reduction.comp + img_upsample.comp +
//                 img_smooth_upsampled.comp + img_addition.comp fused     (K14 + K16 + K7 + K8 + K17)
//
// Streaming ("fast") form, used when the level side S is a multiple of 8: the marches of pyramid_march.h (k_reduce_band,
// k_expand_fast) and, for the metric kernel, a tile of rows brought into LDS by DMA (k_reduce_dma).
//
// Generic form (any S, including the 1..7-pixel tail of the reference's 12-level pyramid):
// one thread per output texel with the shaders' mirror()/out-of-bounds rules applied per tap; with `ref` the shaders' literal
// arithmetic order. k_tiny_tail walks the levels of side <= 32 with it in one launch.
//
// Both forms evaluate exactly the oracle's MUSICA_ORDER_FAST arithmetic. The launches that keep a window of squares in registers
// (launch_expand_sd, launch_rb_sdev, launch_reduce_band_u16_hist, launch_hist_seam) are kernels_expand_sd.hip's.
#include "pyramid_march.h"

namespace musica {

// ======================================================================================
// K5 + K6: out(xo, yo) = sum_m w[m] * ( sum_n w[n] * in(mirror(2xo+m-2), mirror(2yo+n-2)) )
// ======================================================================================

struct RowR {
    float v[8];
    float hl0, hl1;  // columns c0-2, c0-1 of the strip (lane 0 only)
    float hr;        // column c0+512 of the strip (lane 63 only)
};

// One output row from its five input rows (vertical pass in registers, horizontal pass with the
// neighbour columns taken from the adjacent lanes). AUX: cache policy of the store (0 plain, 2 non-temporal).
template <int AUX = 0>
__device__ __forceinline__ void reduce_row(const RowR& r0, const RowR& r1, const RowR& r2, const RowR& r3, const RowR& r4,
                                           const LaneCfg& g, const Buf& ob, uint32_t out_off) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = chain5(r0.v[j], r1.v[j], r2.v[j], r3.v[j], r4.v[j]);
    const float vh0 = chain5(r0.hl0, r1.hl0, r2.hl0, r3.hl0, r4.hl0);
    const float vh1 = chain5(r0.hl1, r1.hl1, r2.hl1, r3.hl1, r4.hl1);
    const float vhr = chain5(r0.hr, r1.hr, r2.hr, r3.hr, r4.hr);
    float vl6 = from_left_lane(v[6]);
    float vl7 = from_left_lane(v[7]);
    float vr0 = from_right_lane(v[0]);
    if (g.lane0) {
        vl6 = g.left_mirror ? v[2] : vh0;  // column -2 -> 2, -1 -> 1 (img_smooth.comp:13)
        vl7 = g.left_mirror ? v[1] : vh1;
    }
    if (g.last_active) vr0 = v[6];         // column S -> S-2 (img_smooth.comp:12)
    else if (g.lane63) vr0 = vhr;
    v4f o;
    o.x = chain5(vl6, vl7, v[0], v[1], v[2]);
    o.y = chain5(v[0], v[1], v[2], v[3], v[4]);
    o.z = chain5(v[2], v[3], v[4], v[5], v[6]);
    o.w = chain5(v[4], v[5], v[6], v[7], vr0);
    llvm_buffer_store_v4f32(o, ob.r, (int)(g.coff + out_off), 0, AUX);   // output columns c/2 .. c/2+3; dropped for lanes right of the image
}

// ---- the metric kernel: img_smooth.comp:18-50 + img_downsample.comp:10-20 of an f32 level -----------------------
// One 256-thread workgroup owns a tile of 512 input columns x kDmaRows output rows. Its 2 * kDmaRows + 3 input rows are
// brought in by LDS-DMA (`buffer_load_dwordx4 ... lds`: 1 KiB per wave-instruction straight from HBM / L2 into LDS, no
// VGPR destination and no register write-back), all of them requested before anything else happens — the four
// wavefronts issue the 2 KiB rows piecewise round-robin — plus one 4-byte DMA for the three halo columns (c0-2, c0-1,
// c0+512) of every row. Each wavefront then waits for its own DMAs, the workgroup meets at ONE barrier, and every
// wavefront computes one output row: five 16-byte-pair LDS reads per lane, the vertical 5-tap pass in registers, the
// horizontal pass with its 2 + 1 neighbour columns from the adjacent lanes by DPP wave shifts (halo columns on lane 0 /
// 63), one non-temporal 16-byte store per lane (the output is not read again by this launch: a plain store leaves the
// lines dirty in the XCD's L2 and their write-back competes with the incoming rows — 18.7 -> 15.9 us at 4096^2). The five rows
// of a tile that no other tile reads come in with the non-temporal policy (15.9 -> 14.85 us, see the loop).
// 22 KiB of LDS per workgroup: 7 workgroups = 154 KiB of rows in flight per CU, and the grid is fine-grained enough
// (4096 workgroups at 4096^2) that the tail of the launch is short. Measured from HBM on MI355X (DESIGN.md §6,
// profiles/r03_*): 4096^2 14.85 us = 0.706 of 8 TB/s (register-staged march of rounds 1-2: 19.3; a plain copy of the same
// traffic shape: 16.1, with non-temporal stores 15.4), 8192^2 51.6 us = 0.81 (march 65.6, copy 58.7).
// Rows the mirror sends outside [0, S) (only when S < 3 could that happen; the fast path needs S >= 8) do not occur; the
// last tile of an image whose So is not a multiple of kDmaRows re-requests valid rows and drops the surplus output rows.
// TAG only separates the launch sites in profiler output: 0 / 1 = level 0 / levels >= 1 of a pipeline that does not fuse
// reduce + band, 2 = stand-alone musica_k_reduce, 4 / 5 = stand-alone rotating over distinct planes at sides <= 4096 / above
// (musica_k_reduce_timed_rot: bench.py's 4096^2 and 8192^2 measurements stay apart in a profiler's per-symbol averages).
constexpr int kDmaRows = 4;                           // output rows per workgroup (one per wavefront)
constexpr int kDmaInRows = 2 * kDmaRows + 3;          // input rows of a tile
constexpr int kDmaPieces = 2 * kDmaInRows;            // 1 KiB pieces (half rows)
constexpr int kDmaPiecesPerWave = (kDmaPieces + kWavesPerBlock - 1) / kWavesPerBlock;
constexpr int kDmaHaloLanes = 24;                     // lanes of the halo DMA (2 per input row, rounded up to a multiple of 8)
static_assert(kDmaRows == kWavesPerBlock && kDmaInRows * 2 <= kDmaHaloLanes, "tile shape");

// Workgroup -> tile for the metric kernel when the strip count is a power of two of at least 2 and the tile rows divide: XCD k (the
// workgroups with linear id % 8 == k) owns a REGION of the image, two strips wide (region_width) and 1 / v of the tile rows tall where
// (strips / 2) v = 8, and walks it row of tiles by row of tiles,
// strip by strip: the tiles left / right and above / below a tile are on the same XCD and dispatched back to back, so the halo
// columns (the neighbouring strip's lines) and the shared halo rows are found in that XCD's L2 — with one strip per XCD (the plain
// mapping at 8 strips) every halo column was another XCD's line and came from the fabric a second time.
// strip PAIRS (quads from 32 strips): 4096^2 = 4 pairs across x 2 halves down, 8192^2 = 8 pairs x the full height, 2048^2 = 2 pairs x 4 quarters.
// Measured at 4096^2 / 8192^2 (us per launch from HBM, fetch + write traffic): pairs 14.62 / 52.5, 87.2 MB; regions of half the strips x
// a quarter of the rows 15.0 / 53.7, 85.2 MB (less fetch, slower); one strip per XCD (round 3) 14.86 / 52.0, 91.3 MB.
__host__ __device__ __forceinline__ unsigned region_width(unsigned strips) { return strips >= 32u ? strips >> 3 : 2u; }
__device__ __forceinline__ Tile xcd_region_tile() {
    const unsigned gx = gridDim.x, gy = gridDim.y;           // strips, tile rows
    const unsigned lin = blockIdx.x + gx * blockIdx.y;
    const unsigned xcd = lin & 7u, j = lin >> 3;
    const unsigned w = region_width(gx);                     // region width in strips
    const unsigned across = gx / w, v = 8u / across;          // regions across x regions down = 8
    const unsigned rh = gy / v;                               // tile rows per region
    const unsigned rx = xcd % across, ry = xcd / across;
    Tile t;
    t.strip = (int)(rx * w + j % w);
    t.segblock = (int)(ry * rh + j / w);
    return t;
}

// M0 = LDS byte address the wave-instruction writes to (wave-uniform); lane l lands at M0 + 16 l (dwordx4) / M0 + 4 l (dword).
// An asm load is invisible to hipcc's s_waitcnt bookkeeping: the kernel waits with its own vmcnt(0) below.
// (M0 is compiler-reserved: it is saved and restored inside the statement that changes it.)
__device__ __forceinline__ void dma16(const Buf& b, uint32_t voff, uint32_t lds_byte) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_byte), "v"(voff), "s"(b.r) : "memory");
}
// the same with the non-temporal cache policy: for bytes no other workgroup will ask for
__device__ __forceinline__ void dma16_nt(const Buf& b, uint32_t voff, uint32_t lds_byte) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen nt lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_byte), "v"(voff), "s"(b.r) : "memory");
}

template <int TAG>
__global__ __launch_bounds__(kBlockThreads) void k_reduce_dma(const float* __restrict__ in, float* __restrict__ out,
                                                              int S, int pitch, size_t in_plane, int So, int opitch,
                                                              size_t out_plane, int swz) {
    __shared__ __attribute__((aligned(16))) float tile_s[kDmaInRows * kStripCols + kDmaHaloLanes * 4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const Tile tile = swz == 2 ? xcd_region_tile() : xcd_tile(swz);
    const int yo0 = tile.segblock * kDmaRows;
    const Buf ib = make_buf(in + (size_t)blockIdx.z * in_plane, in_plane * 4);
    const Buf ob = make_buf(out + (size_t)blockIdx.z * out_plane, out_plane * 4);
    const LaneCfg g = make_cfg(tile.strip, lane, S);
    const int c0 = tile.strip * kStripCols;
    const int hi = S - 1;
    const uint32_t rb = (uint32_t)pitch * 4u, orb = (uint32_t)opitch * 4u;
    const uint32_t lds0 = (uint32_t)(uintptr_t)tile_s;   // LDS byte address of the tile (low half of the flat address)
    // local row k of the tile = input row mirror(2 * yo0 - 2 + k) (img_smooth.comp:10-16), kept inside the image
    // halo columns of every row as two aligned 16-byte pieces — columns c0-4 .. c0-1 and c0+512 .. c0+515 — by ONE dwordx4 DMA of
    // 2 x 11 lanes (wavefront 0; entry 2 k + side, 4 floats each). Until round 4 a dword DMA gathered the three columns a row needs
    // one by one: 33 requests per tile, each a fabric request of its own on a line of the neighbouring strip (+9 % of fetch, PMC);
    // 22 now, and with the region mapping below the neighbour's line is usually in this XCD's L2 already.
    if (wave == 0 && lane < kDmaHaloLanes) {
        const int k = lane >> 1, side = lane & 1;
        const int y = min(max(mirror_idx(2 * yo0 - 2 + min(k, kDmaInRows - 1), hi), 0), hi);
        const int col = side ? c0 + kStripCols : c0 - 4;
        const bool ok = k < kDmaInRows && col >= 0 && col < S;
        dma16(ib, ok ? (uint32_t)y * rb + (uint32_t)col * 4u : kOob, lds0 + (uint32_t)(kDmaInRows * kStripCols) * 4u);
    }
    const uint32_t lane_off = (uint32_t)(c0 + lane * 4) * 4u;   // a piece = 256 columns, 4 per lane
#pragma unroll
    for (int i = 0; i < kDmaPiecesPerWave; i++) {
        const int q = min(i * kWavesPerBlock + wave, kDmaPieces - 1);   // a wave without a last piece repeats the tile's last one
        const int k = q >> 1, half = q & 1;
        const int y = min(max(mirror_idx(2 * yo0 - 2 + k, hi), 0), hi);
        const bool ok = c0 + half * 256 + lane * 4 < S;
        const uint32_t src = ok ? (uint32_t)y * rb + lane_off + (uint32_t)half * 1024u : kOob, dst = lds0 + (uint32_t)(k * kStripCols + half * 256) * 4u;
        // rows 0-2 and 8-10 of a tile are also the tile above's / below's: default policy, so the second reader finds them in the
        // XCD's L2; rows 3-7 are read by nobody else: non-temporal, they do not push the shared rows out (a CU's seven tiles x 32 CUs
        // are 4.9 MB in flight against 4 MiB of L2). 4096^2: 15.9 -> 14.85 us, 8192^2: 55.3 -> 51.6 us; nt on every row: 17.9 us.
        if (k >= 3 && k < 2 * kDmaRows) dma16_nt(ib, src, dst);   // wave-uniform
        else dma16(ib, src, dst);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const float* hal = tile_s + kDmaInRows * kStripCols;
    RowR w[5];
#pragma unroll
    for (int r = 0; r < 5; r++) {
        const int k = 2 * wave + r;
        const float4 a = *reinterpret_cast<const float4*>(tile_s + k * kStripCols + lane * 8);
        const float4 b = *reinterpret_cast<const float4*>(tile_s + k * kStripCols + lane * 8 + 4);
        w[r].v[0] = a.x; w[r].v[1] = a.y; w[r].v[2] = a.z; w[r].v[3] = a.w; w[r].v[4] = b.x; w[r].v[5] = b.y; w[r].v[6] = b.z; w[r].v[7] = b.w;
        w[r].hl0 = hal[8 * k + 2]; w[r].hl1 = hal[8 * k + 3]; w[r].hr = hal[8 * k + 4];   // columns c0-2, c0-1 | c0+512
    }
    const int yo = yo0 + wave;
    if (yo < So) reduce_row<2>(w[0], w[1], w[2], w[3], w[4], g, ob, (uint32_t)yo * orb);   // wave-uniform
}

// One thread per output texel, any S >= 1. OOB loads (only reachable when S < 3, where the
// reference's unclamped mirror() leaves the image) return 0.
// Branch-free on purpose: the load always happens (texel (0, 0) stands in for an out-of-image tap) and the test only selects, so
// the 25 taps of a stencil are requested together instead of one branch + load + wait each (k_tiny_tail: 41 -> 14 us).
__device__ __forceinline__ float ld0(const float* __restrict__ im, int pitch, int S, int x, int y) {
    const bool in = x >= 0 && y >= 0 && x < S && y < S;
    const float v = im[(size_t)(in ? y : 0) * pitch + (in ? x : 0)];
    return in ? v : 0.0f;
}

// ---- the shaders' literal arithmetic order (MUSICA_FLAG_REFERENCE_ORDER) ---------------------------------------
// img_smooth.comp:32-45 / img_smooth_upsampled.comp:32-45 accumulate the 25 taps m (x) outer, n (y) inner,
// `pixel += weight[m] * weight[n] [* 4.0] * load`, starting from 0; img_sdev.comp:17-30 the 25 squares likewise.
// The generic kernels take a wave-uniform `ref` argument and then evaluate exactly that sequence (the oracle's
// MUSICA_ORDER_REFERENCE); speed is secondary here.
__device__ __forceinline__ float w5(int i) { return i == 0 ? W0 : i == 1 ? W1 : i == 2 ? W2 : i == 3 ? W3 : W4; }

__device__ __forceinline__ float smooth_literal(const float* __restrict__ in, int pitch, int S, int x, int y) {
    const int hi = S - 1;
    float pixel = 0.0f;
#pragma unroll
    for (int m = 0; m < 5; m++) {
        const int xm = mirror_idx(x + m - 2, hi);
#pragma unroll
        for (int n = 0; n < 5; n++) pixel = pixel + (w5(m) * w5(n)) * ld0(in, pitch, S, xm, mirror_idx(y + n - 2, hi));   // img_smooth.comp:43
    }
    return pixel;
}

// smooth + downsample at coarse (xo, yo) for any S (generic form)
__device__ __forceinline__ float reduce_generic_at(const float* __restrict__ in, int pitch, int S, int xo, int yo, int ref) {
    if (ref) return smooth_literal(in, pitch, S, 2 * xo, 2 * yo);   // img_downsample.comp:15 of the literally smoothed image
    const int hi = S - 1;
    float v[5];
#pragma unroll
    for (int m = 0; m < 5; m++) {
        const int x = mirror_idx(2 * xo + m - 2, hi);   // outside the image (S < 3): five zero taps, chain5 = +0
        v[m] = chain5(ld0(in, pitch, S, x, mirror_idx(2 * yo - 2, hi)), ld0(in, pitch, S, x, mirror_idx(2 * yo - 1, hi)),
                      ld0(in, pitch, S, x, mirror_idx(2 * yo, hi)), ld0(in, pitch, S, x, mirror_idx(2 * yo + 1, hi)),
                      ld0(in, pitch, S, x, mirror_idx(2 * yo + 2, hi)));
    }
    return chain5(v[0], v[1], v[2], v[3], v[4]);
}
__global__ void k_reduce_generic(const float* __restrict__ in, float* __restrict__ out, int S, int pitch,
                                 size_t in_plane, int So, int opitch, size_t out_plane, int ref) {
    const int xo = blockIdx.x * blockDim.x + threadIdx.x;
    const int yo = blockIdx.y * blockDim.y + threadIdx.y;
    if (xo >= So || yo >= So) return;
    in += (size_t)blockIdx.z * in_plane;
    out += (size_t)blockIdx.z * out_plane;
    out[(size_t)yo * opitch + xo] = reduce_generic_at(in, pitch, S, xo, yo, ref);
}

// reduce + band of a level in one march (reduce_band_block, pyramid_march.h) as a launch of its own; grid: stream_grid()
template <bool U16>
__global__ __launch_bounds__(kBlockThreads, 4) void k_reduce_band(const void* __restrict__ fine, float* __restrict__ down, float* __restrict__ band,
                                                               int S, int pitch, size_t plane, int Sc, int cpitch, size_t cplane,
                                                               int rows_per_wave, const uint32_t* __restrict__ minmax, int min_chain_exact,
                                                               uint16_t* __restrict__ le090, int swz) {
    reduce_band_block<U16>(fine, down, band, S, pitch, plane, Sc, cpitch, cplane, rows_per_wave, minmax, min_chain_exact, le090, xcd_tile(swz), (int)blockIdx.z);
}

// lowpass value at fine (x, y) for any S (generic form).
__device__ __forceinline__ float lowpass_generic(const float* __restrict__ coarse, int cpitch, int Sc, int S, int x, int y, int ref) {
    if (ref) {   // img_smooth_upsampled.comp:32-45 on the zero-inserted image of img_upsample.comp (odd texels: 0, Q2), literally
        float pixel = 0.0f;
#pragma unroll
        for (int m = 0; m < 5; m++) {
            const int j = coarse_of_fine(x + m - 2, S);
#pragma unroll
            for (int n = 0; n < 5; n++) {
                const int k = coarse_of_fine(y + n - 2, S);
                const float tap = ld0(coarse, cpitch, Sc, j, k);   // j, k < 0 (odd fine index: the inserted zero) read 0
                pixel = pixel + ((w5(m) * w5(n)) * 4.0f) * tap;   // :43
            }
        }
        return pixel;
    }
    float V[5];
#pragma unroll
    for (int m = 0; m < 5; m++) {
        const int j = coarse_of_fine(x + m - 2, S);   // -1 (an inserted zero column): five zero taps, the sum is +0
        float acc = 0.0f;
#pragma unroll
        for (int n = 0; n < 5; n++) {
            const int k = coarse_of_fine(y + n - 2, S);
            const float w = n == 0 ? W0 : n == 1 ? W1 : n == 2 ? W2 : n == 3 ? W3 : W4;
            const float t = w * ld0(coarse, cpitch, Sc, j, k);   // j, k < 0 read 0
            acc = n == 0 ? t : acc + t;
        }
        V[m] = acc;
    }
    return 4.0f * chain5(V[0], V[1], V[2], V[3], V[4]);
}

__global__ void k_band_generic(const float* __restrict__ fine, const float* __restrict__ coarse, float* __restrict__ band,
                               int S, int pitch, size_t plane, int Sc, int cpitch, size_t cplane, int ref) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= S || y >= S) return;
    fine += (size_t)blockIdx.z * plane;
    band += (size_t)blockIdx.z * plane;
    coarse += (size_t)blockIdx.z * cplane;
    const float low = lowpass_generic(coarse, cpitch, Sc, S, x, y, ref);
    band[(size_t)y * pitch + x] = fine[(size_t)y * pitch + x] - low;
}

// lowpass only (debugProcess' red_lowpass_i / exp_lowpass_i dumps, kernel-level tests)
__global__ void k_lowpass_generic(const float* __restrict__ coarse, float* __restrict__ low, int S, int pitch, size_t plane,
                                  int Sc, int cpitch, size_t cplane, int ref) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= S || y >= S) return;
    low += (size_t)blockIdx.z * plane;
    coarse += (size_t)blockIdx.z * cplane;
    low[(size_t)y * pitch + x] = lowpass_generic(coarse, cpitch, Sc, S, x, y, ref);
}

// linearFunction() of noise_reduction.comp:24-31 — m * x, not m * (x - p1.x).
__device__ __forceinline__ float nr_factor(float c, float lowCnr, float lowFactor, float highCnr, float highFactor) {
    if (c < lowCnr) return lowFactor;
    else if (c > highCnr) return highFactor;
    const float m = (highFactor - lowFactor) / (highCnr - lowCnr);
    return m * c + lowFactor;
}

__device__ __forceinline__ void curve_to_lds_2d(CurveLds& tab, const DevCurve* __restrict__ src) {
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    for (int i = tid; i < kCurveCap; i += blockDim.x * blockDim.y) {
        tab.x[i] = src->x[i]; tab.y[i] = src->y[i]; tab.m[i] = src->m[i];
    }
    if (tid == 0) { tab.count = src->count; tab.monotone = src->monotone; }
}

// band * gain [* nr] at one texel (generic form)
template <int GAIN, bool NR>
__device__ __forceinline__ float exp_band_at(const ExpandArgs& a, const CurveLds& tab, int img, int x, int y) {
    const size_t o = (size_t)img * a.plane + (size_t)y * a.pitch + x;
    const float s = (GAIN != GAIN_CONST) ? a.sdev[o] : 0.0f;
    float p = a.band[o] * gain_of<GAIN>(s, a.high, tab);
    if (NR) {
        const int cx = x / a.cnrScale, cy = y / a.cnrScale;
        const float c = ((cx < a.cnrS && cy < a.cnrS) ? a.cnr[(size_t)img * a.cnrPlane + (size_t)cy * a.cnrPitch + cx] : 0.0f) * kMaxCnrValue;
        p = p * nr_factor(c, a.lowCnr, a.lowFactor, a.highCnr, a.highFactor);
    }
    return p;
}

template <int GAIN, bool NR>
__global__ void k_expand_generic(ExpandArgs a) {
    __shared__ CurveLds tab;
    const int img = blockIdx.z;
    if (GAIN == GAIN_CURVE) {
        curve_to_lds_2d(tab, a.curves + (size_t)img * a.curve_stride);
        __syncthreads();
    }
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= a.S || y >= a.S) return;
    const float low = lowpass_generic(a.prev + (size_t)img * a.cplane, a.cpitch, a.Sc, a.S, x, y, a.ref_order);
    a.recon[(size_t)img * a.plane + (size_t)y * a.pitch + x] = low + exp_band_at<GAIN, NR>(a, tab, img, x, y);
}

// band after contrast curve (+ noise reduction): what img_addition.comp reads as inputImageB
// (debugProcess' exp_bandpass_i dump; not materialised on the hot path).
template <int GAIN, bool NR>
__global__ void k_exp_band_generic(ExpandArgs a) {
    __shared__ CurveLds tab;
    const int img = blockIdx.z;
    if (GAIN == GAIN_CURVE) {
        curve_to_lds_2d(tab, a.curves + (size_t)img * a.curve_stride);
        __syncthreads();
    }
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= a.S || y >= a.S) return;
    a.recon[(size_t)img * a.plane + (size_t)y * a.pitch + x] = exp_band_at<GAIN, NR>(a, tab, img, x, y);
}

// ---- the tiny tail of the pyramid in one launch ------------------------------------------------------------------
// Levels whose side is at most 32 (the last four or five of a full-depth pyramid: 24, 12, 6, 3, 2 for the reference's
// 3072^2 / L = 12) are a few hundred texels each, yet every one costs three or four launches of ~5 us (reduce, band, expand: 14
// launches, 72 us of a 270 us step at 3072^2 / L12). One 1024-thread workgroup per image walks them here: reduce and band of levels
// T .. L-1, then expand L-1 .. T (constant gain: these levels are above the cnr level), a texel per thread and phase, with the
// SAME device functions as the per-level generic launches (reduce_generic_at, lowpass_generic: same bits) and a workgroup
// barrier between dependent phases.
// The images live in LDS while the workgroup works on them (dense rows; ~4100 floats for sides 32, 16, 8, ..: a phase reads 25
// taps per texel — from the XCD's L2, where the workgroup's own stores land, that is 25 round trips of ~1 us) and every result is
// also stored to its global image (the getters, and the expand slot of level T - 1, read those).
constexpr int kTailPool = 3 * (kTailSide * kTailSide + (kTailSide / 2) * (kTailSide / 2) * 2) + 64;   // fine + band + recon of every level (sum of squares < 1.5 x the first)
__global__ __launch_bounds__(1024) void k_tiny_tail(const TailArgs a) {
    __shared__ float pool[kTailPool];
    // side of level k (k = n: the coarsest image) and where its fine, band and reconstruction images sit in the pool. Rolled
    // loops over LDS tables on purpose: unrolled per level, the three stencils are ~100 KB of code that runs once (44 us per
    // launch, most of it instruction fetch).
    __shared__ int side[kTailMax + 1], offF[kTailMax + 1], offB[kTailMax], offR[kTailMax];
    const size_t img = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x, n = a.n;
    if (tid == 0) {
        int o = 0;
        for (int k = 0; k <= n; k++) { side[k] = k < n ? a.l[k].S : a.Sl; offF[k] = o; o += side[k] * side[k]; }
        for (int k = 0; k < n; k++) { offB[k] = o; o += side[k] * side[k]; offR[k] = o; o += side[k] * side[k]; }
    }
    {
        const TailLevel& f = a.l[0];
        const float* fine = f.fine + img * f.plane;
        for (int i = tid; i < f.S * f.S; i += nt) {
            const int y = i / f.S, x = i - y * f.S;
            pool[i] = fine[(size_t)y * f.pitch + x];   // offF[0] = 0
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < n; k++) {
        const int S = side[k], Sc = side[k + 1];
        const float* fineL = pool + offF[k];
        float* downL = pool + offF[k + 1];
        for (int i = tid; i < Sc * Sc; i += nt) {
            const int yo = i / Sc, xo = i - yo * Sc;
            downL[i] = reduce_generic_at(fineL, S, S, xo, yo, a.ref);
        }
        __syncthreads();
        float* bandL = pool + offB[k];
        for (int i = tid; i < S * S; i += nt) {
            const int y = i / S, x = i - y * S;
            bandL[i] = fineL[i] - lowpass_generic(downL, Sc, Sc, S, x, y, a.ref);
        }
    }
#pragma unroll 1
    for (int k = n - 1; k >= 0; k--) {
        __syncthreads();   // the coarser reconstruction is complete (and, the first time, every band image)
        const int S = side[k], Sc = side[k + 1];
        const float* prevL = pool + (k + 1 == n ? offF[k + 1] : offR[k + 1]);   // src/vk_processing.cpp:930-934
        const float* bandL = pool + offB[k];
        float* reconL = pool + offR[k];
        const float high = a.l[k].high;
        for (int i = tid; i < S * S; i += nt) {
            const int y = i / S, x = i - y * S;
            const float low = lowpass_generic(prevL, Sc, Sc, S, x, y, a.ref);
            reconL[i] = low + bandL[i] * high;   // contrast_curve_apply.comp:61 (two-point curve), img_addition.comp:15
        }
    }
    __syncthreads();
    // every image to its global plane, once, behind the last phase
#pragma unroll 1
    for (int k = 0; k < n; k++) {
        const TailLevel& f = a.l[k];
        const bool last = k + 1 == n;
        const int S = side[k], Sc = side[k + 1], cpitch = last ? a.lpitch : a.l[k + 1].pitch;
        const size_t cplane = last ? a.lplane : a.l[k + 1].plane;
        float* down = f.down + img * cplane;
        for (int i = tid; i < Sc * Sc; i += nt) {
            const int yo = i / Sc, xo = i - yo * Sc;
            down[(size_t)yo * cpitch + xo] = pool[offF[k + 1] + i];
        }
        float* band = f.band + img * f.plane;
        float* recon = f.recon + img * f.plane;
        for (int i = tid; i < S * S; i += nt) {
            const int y = i / S, x = i - y * S;
            band[(size_t)y * f.pitch + x] = pool[offB[k] + i];
            recon[(size_t)y * f.pitch + x] = pool[offR[k] + i];
        }
    }
}

// ======================================================================================
// host-side launchers
// ======================================================================================

void launch_tiny_tail(hipStream_t st, const TailArgs& a, int batch) {
    hipLaunchKernelGGL(k_tiny_tail, dim3(batch), dim3(1024), 0, st, a);
}

static inline dim3 generic_grid(int S, int batch) { return dim3((S + 31) / 32, (S + 7) / 8, batch); }
static const dim3 kGenericBlock(32, 8, 1);

static inline bool fast_ok(int S) { return S >= 8 && (S % 8) == 0; }

// tag: launch site (see k_reduce_dma)
// regions = 0 (MUSICA_XCD_REGIONS=0): the round-3 tile mapping of the metric kernel
void launch_reduce(hipStream_t st, const float* in, const LevelDesc& li, float* out, const LevelDesc& lo, int batch, bool force_generic, int tag,
                   int swz_on, int regions, int ref) {
    if (fast_ok(li.S) && !force_generic) {
        const int strips = (li.S + kStripCols - 1) / kStripCols;
        const dim3 grid(strips, (lo.S + kDmaRows - 1) / kDmaRows, batch);
        // 8 k strips: workgroup id % 8 == strip % 8 already gives every strip one XCD, tile above tile in dispatch order; otherwise
        // the XCD-aware mapping does (2048^2: 6.0 -> 5.05 us; it costs 1.5 us at 4096^2 where the plain mapping has that property).
        // Round 4: where the geometry allows, 2-D regions per XCD (xcd_region_tile): horizontal neighbours share an L2 as well.
        int swz = (strips % 8) != 0 ? swz_on : 0;
        {
            const unsigned gx = (unsigned)strips, gy = grid.y;
            const bool pow2 = gx >= 2 && (gx & (gx - 1)) == 0 && gx <= 32;
            const unsigned w = region_width(gx), across = pow2 ? gx / w : 1u, v = pow2 ? 8u / across : 1u;
            if (pow2 && across * v == 8u && gy % v == 0 && swz_on && regions) swz = 2;
        }
        auto* kern = tag == 0 ? k_reduce_dma<0> : tag == 1 ? k_reduce_dma<1> : tag == 2 ? k_reduce_dma<2> : tag == 4 ? k_reduce_dma<4> : k_reduce_dma<5>;
        hipLaunchKernelGGL(kern, grid, dim3(kBlockThreads), 0, st, in, out, li.S, li.pitch, li.plane, lo.S, lo.pitch, lo.plane, swz);
    } else {
        hipLaunchKernelGGL(k_reduce_generic, generic_grid(lo.S, batch), kGenericBlock, 0, st, in, out, li.S, li.pitch,
                           li.plane, lo.S, lo.pitch, lo.plane, ref);
    }
}

void launch_reduce_band_u16(hipStream_t st, const uint16_t* px, float* down, float* band, const LevelDesc& lf, const LevelDesc& lc, int batch,
                            int rows_per_wave, const uint32_t* minmax, int min_chain_exact, uint16_t* le090, int swz) {
    hipLaunchKernelGGL(k_reduce_band<true>, stream_grid(lf.S, lc.S, rows_per_wave, batch), dim3(kBlockThreads), 0, st, (const void*)px, down, band, lf.S,
                       lf.pitch, lf.plane, lc.S, lc.pitch, lc.plane, rows_per_wave, minmax, min_chain_exact, le090, swz);
}
// levels >= 1 (f32 fine image); the side must be a multiple of 8 and at least 16 (the caller checks)
void launch_reduce_band(hipStream_t st, const float* fine, float* down, float* band, const LevelDesc& lf, const LevelDesc& lc, int batch, int rows_per_wave, int swz) {
    hipLaunchKernelGGL(k_reduce_band<false>, stream_grid(lf.S, lc.S, rows_per_wave, batch), dim3(kBlockThreads), 0, st, (const void*)fine, down, band, lf.S,
                       lf.pitch, lf.plane, lc.S, lc.pitch, lc.plane, rows_per_wave, (const uint32_t*)nullptr, 0, (uint16_t*)nullptr, swz);
}
// band of a level that does not take the fused reduce + band march (sides that are not a multiple of 8, generic / literal-order contexts)
void launch_band(hipStream_t st, const float* fine, const float* coarse, float* band, const LevelDesc& lf, const LevelDesc& lc, int batch, int ref) {
    hipLaunchKernelGGL(k_band_generic, generic_grid(lf.S, batch), kGenericBlock, 0, st, fine, coarse, band, lf.S, lf.pitch,
                       lf.plane, lc.S, lc.pitch, lc.plane, ref);
}

void launch_lowpass(hipStream_t st, const float* coarse, float* low, const LevelDesc& lf, const LevelDesc& lc, int batch, int ref) {
    hipLaunchKernelGGL(k_lowpass_generic, generic_grid(lf.S, batch), kGenericBlock, 0, st, coarse, low, lf.S, lf.pitch, lf.plane,
                       lc.S, lc.pitch, lc.plane, ref);
}

template <int GAIN, bool NR>
static void launch_expand_t(hipStream_t st, const ExpandArgs& a, int batch, bool force_generic) {
    if (GAIN == GAIN_CURVE && !a.sdev) {   // the level's sdev image is not stored: the launch computes sdev itself (k_expand_fast<.., SD>, kernels_expand_sd.hip)
        launch_expand_sd(st, a, NR, batch);
        return;
    }
    if (fast_ok(a.S) && !force_generic) {
        const dim3 grid = stream_grid(a.S, a.Sc, a.rows_per_wave, batch);
        if (GAIN == GAIN_CURVE && NR && a.ghist) {   // level 0 with the gradation histogram on board (the caller checked cnrScale == 8 and passes le090)
            // W = 4: register allocation capped at 128 (4 wavefronts per SIMD) against 143 registers and 3 wavefronts
            // a.chist: a tile side (S / 4) of at least a strip and at least the rows of a workgroup (the caller checks)
            if (a.chist) hipLaunchKernelGGL((k_expand_fast<GAIN_CURVE, true, true, 4, true>), grid, dim3(kBlockThreads), 0, st, a);
            else hipLaunchKernelGGL((k_expand_fast<GAIN_CURVE, true, true, 4>), grid, dim3(kBlockThreads), 0, st, a);
        }
        else hipLaunchKernelGGL((k_expand_fast<GAIN, NR, false, NR ? 4 : 1>), grid, dim3(kBlockThreads), 0, st, a);   // NR: 129 registers wanted, capped at 128 (4 wavefronts per SIMD)
    } else {
        hipLaunchKernelGGL((k_expand_generic<GAIN, NR>), generic_grid(a.S, batch), kGenericBlock, 0, st, a);
    }
}

void launch_expand(hipStream_t st, const ExpandArgs& a, int gain_mode, bool nr, int batch, bool force_generic) {
    if (gain_mode == GAIN_CONST) launch_expand_t<GAIN_CONST, false>(st, a, batch, force_generic);
    else if (gain_mode == GAIN_RANGE) launch_expand_t<GAIN_RANGE, false>(st, a, batch, force_generic);
    else if (nr) launch_expand_t<GAIN_CURVE, true>(st, a, batch, force_generic);
    else launch_expand_t<GAIN_CURVE, false>(st, a, batch, force_generic);
}

void launch_exp_band(hipStream_t st, const ExpandArgs& a, int gain_mode, bool nr, int batch) {
    const dim3 g = generic_grid(a.S, batch);
    if (gain_mode == GAIN_CONST) hipLaunchKernelGGL((k_exp_band_generic<GAIN_CONST, false>), g, kGenericBlock, 0, st, a);
    else if (gain_mode == GAIN_RANGE) hipLaunchKernelGGL((k_exp_band_generic<GAIN_RANGE, false>), g, kGenericBlock, 0, st, a);
    else if (nr) hipLaunchKernelGGL((k_exp_band_generic<GAIN_CURVE, true>), g, kGenericBlock, 0, st, a);
    else hipLaunchKernelGGL((k_exp_band_generic<GAIN_CURVE, false>), g, kGenericBlock, 0, st, a);
}

}  // namespace musica
