// study_device.h — what the study's kernels share on the device (kernels_similarity.hip, kernels_scales.hip, kernels_joint.hip,
// kernels_displace.hip, kernels_covariance.hip, kernels_ensemble.hip, kernels_details.hip, kernels_edges.hip, kernels_gratings.hip,
// kernels_points.hip, kernels_gain.hip, kernels_levels.hip, kernels_gradients.hip, kernels_order.hip, kernels_scatter.hip, kernels_reach.hip, kernels_observer.hip, kernels_blobs.hip, kernels_spectrum.hip, kernels_cooccurrence.hip, kernels_granulometry.hip, kernels_contours.hip): the address-space typedefs, the
// reductions and their ONE order, the workgroup's prefix sum, the
// 64 x 64 tile of a region, the pixel words of the kernels that stream a u16 plane and the insertion body of the patch relations
// (insert_patches), the packed byte windows of k_displace and k_cov_add, the staged windows of k_gradients and k_order (stage_windows), the one-sided window with a clipped halo of k_cooccurrence, k_granulometry and k_contour_mask (stage_halo_window), and the
// per-window SSIM terms.
#pragma once

#include <type_traits>

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
typedef __attribute__((address_space(1))) uint32_t GlobalU32;

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

// INTEGER sums only, where any order gives the same bits: every 32-bit argument summed over its wavefront by DPP adds, in place. The
// wavefront's LAST lane (wave_last) ends with the sum; the other lanes hold partial sums. All 64 lanes must be active. The six steps
// are the scan of the compiler's own wavefront reductions on gfx9: row_shr 1, 2, 4, 8 inside the rows of 16 lanes (a lane without a
// source adds 0), then row_bcast15 into rows 1 and 3 and row_bcast31 into rows 2 and 3: adds with a DPP operand, no LDS traffic,
// where the __shfl_down tree of wave_sum is six dependent ds_bpermute_b32 a value.
template <int CTRL, int ROWS, typename T>
__device__ __forceinline__ void wave_isum_step(T& v) {
    static_assert(sizeof(T) == 4 && std::is_integral<T>::value, "32-bit integers");
    v = (T)((uint32_t)v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xF, false));
}
template <typename... T>
__device__ __forceinline__ void wave_isum(T&... v) {
    (wave_isum_step<0x111, 0xF>(v), ...);   // row_shr:1
    (wave_isum_step<0x112, 0xF>(v), ...);   // row_shr:2
    (wave_isum_step<0x114, 0xF>(v), ...);   // row_shr:4
    (wave_isum_step<0x118, 0xF>(v), ...);   // row_shr:8
    (wave_isum_step<0x142, 0xA>(v), ...);   // row_bcast15 into rows 1 and 3
    (wave_isum_step<0x143, 0xC>(v), ...);   // row_bcast31 into rows 2 and 3
}
__device__ __forceinline__ bool wave_last() { return (threadIdx.x & 63) == 63; }
// The same six steps with an UNSIGNED maximum in place of the add (a lane without a source takes max(v, 0) = v): the wavefront's last
// lane ends with the largest argument. All 64 lanes must be active.
template <int CTRL, int ROWS>
__device__ __forceinline__ void wave_umax_step(uint32_t& v) {
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xF, false);
    v = o > v ? o : v;
}
__device__ __forceinline__ void wave_umax(uint32_t& v) {
    wave_umax_step<0x111, 0xF>(v);
    wave_umax_step<0x112, 0xF>(v);
    wave_umax_step<0x114, 0xF>(v);
    wave_umax_step<0x118, 0xF>(v);
    wave_umax_step<0x142, 0xA>(v);
    wave_umax_step<0x143, 0xC>(v);
}

// The exclusive prefix of v over the workgroup's threads (thread order; k_scatter_rows, k_reach_rows); wave_tot: one word a wavefront,
// free again on return. total: where given, every thread also gets the sum over the whole workgroup.
template <typename U>
__device__ __forceinline__ U block_scan_exclusive(U v, U* wave_tot, U* total = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    U inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const U o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    U before = 0;
    for (int w = 0; w < wave; w++) before += wave_tot[w];
    if (total) {
        U all = before;
        for (int w = wave; w < (int)(blockDim.x >> 6); w++) all += wave_tot[w];
        *total = all;
    }
    __syncthreads();
    return before + inc - v;
}

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

// ---- pixel words (k_alter_details, k_alter_edges, k_alter_gratings, k_alter_gain) ---------------------------------------------------
// A thread of these kernels moves chunks of V consecutive u16 pixels of a row with one load and one store: V = 8 (16 bytes) where the
// side is a multiple of 8 and every plane is 16-byte aligned, else 2 under the same condition for 4 bytes, else single pixels (image 1
// of a batch with odd N^2 starts on a 2-byte boundary only). With n % V == 0 a chunk starts inside the plane or lies outside it entirely.
template <int V> struct PixelWord;
template <> struct PixelWord<8> { typedef uint4 type; };
template <> struct PixelWord<2> { typedef uint32_t type; };
template <> struct PixelWord<1> { typedef uint16_t type; };
template <int V>
union PixelChunk {
    typename PixelWord<V>::type w;
    uint16_t px[V];
};

// n % v == 0 and every plane (or table read a chunk at a time) aligned to 2 v bytes
template <typename... P>
inline bool pixels_aligned(int n, int v, const P*... planes) {
    return n % v == 0 && ((reinterpret_cast<uintptr_t>(planes) % (2 * v) == 0) && ...);
}

// launch(std::integral_constant<int, V>) for the widest V the side and the planes allow
template <typename Launch, typename... P>
inline void launch_by_width(Launch&& launch, int n, const P*... planes) {
    if (pixels_aligned(n, 8, planes...)) launch(std::integral_constant<int, 8>());
    else if (pixels_aligned(n, 2, planes...)) launch(std::integral_constant<int, 2>());
    else launch(std::integral_constant<int, 1>());
}

// ---- the insertion body of the patch relations (k_alter_details, k_alter_edges, k_alter_gratings, k_alter_points) ---------------------------------
// ONE launch, 2 B read + 2 B written per pixel: a pixel inside a listed patch is changed by the relation's rule, every other pixel is
// copied. The patches of a list (discs in their boxes, plates) lie inside the plane and are pairwise disjoint (the callers check), so a
// pixel belongs to at most one. A workgroup of kStudyThreads threads owns a 64 x 64 tile of the plane (tile_geom).
//   bin      the threads stride over the packed list and append to an LDS list the patches whose square (centre +- Entry::r) meets the
//            tile, through an LDS counter; the order of the appends does not matter because a pixel meets at most one patch. The
//            relation's file argues and asserts the CAPACITY R::kTileCap of a tile's list; an append past it would be dropped, never
//            written.
//   stage    a relation may stage more behind the list, in LDS of its own (R::stage: the gratings' waves).
//   stream   a thread moves chunks of V consecutive pixels of a row (pixel words above); consecutive lanes take consecutive chunks.
//            Two passes, unrolled: every load of a thread is in flight before the first is used. A tile with an empty list is a pure
//            copy; elsewhere a chunk is tested against the listed patches' squares first and only the chunks that meet one set up the
//            relation's row state (R::row) and apply its rule to their V pixels (R::pixel).
// Nothing outside the two planes (and what R::stage reads) is read, nothing outside `out` written; the planes must not overlap.
// A relation R supplies: Packed, the list's item as it travels; Entry, its LDS form, which begins with int x, y, r (the centre in tile
// coordinates and the reach of the square); kTileCap; meets(packed, tile, entry&): whether the item meets the tile, and if so its entry;
// stage(list, m, extra...) -> Staged (empty where there is nothing to stage); Row and row(entry, j, dy, tx, staged): the state of a
// chunk at tile column tx of the row dy below the centre of patch j; pixel(entry, row&, dx, px&): pixel dx right of the centre.
template <typename R, int V, typename... Extra>
__device__ __forceinline__ void insert_patches(const uint16_t* __restrict__ src, uint16_t* __restrict__ out, int n,
                                               const typename R::Packed* __restrict__ items, int count, Extra... extra) {
    typedef typename PixelWord<V>::type __attribute__((may_alias)) Word;
    typedef typename R::Entry Entry;
    constexpr int ROW = kSimTile / V;                            // chunks per tile row
    constexpr int TRIPS = kSimTile * ROW / kStudyThreads;        // chunks per thread
    __shared__ Entry list[R::kTileCap];
    __shared__ int listed;
    const int tiles = (n + kSimTile - 1) / kSimTile;
    const TileGeom t = tile_geom(blockIdx.x, tiles, n, n);
    if (threadIdx.x == 0) listed = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < count; i += kStudyThreads) {
        // The item whole, before the test: a field fetched behind the test is a second load that is still pending where the test fails,
        // and the wait for it then lands behind the first chunk's store (0.45 us of k_alter_edges<8> at 3072^2).
        const typename R::Packed p = items[i];
        Entry e;
        if (!R::meets(p, t, e)) continue;
        const int slot = atomicAdd(&listed, 1);
        if (slot < R::kTileCap) list[slot] = e;
    }
    __syncthreads();
    const int m = min(listed, R::kTileCap);
    const typename R::Staged staged = R::stage(list, m, extra...);

    PixelChunk<V> loaded[TRIPS];
#pragma unroll
    for (int k = 0; k < TRIPS; k++) {
        const int e = k * kStudyThreads + (int)threadIdx.x;
        const int ty = e / ROW, tx = (e - ty * ROW) * V;
        if (ty < t.th && tx < t.tw) loaded[k].w = *reinterpret_cast<const Word*>(src + (size_t)(t.y0 + ty) * n + (t.x0 + tx));
    }
#pragma unroll
    for (int k = 0; k < TRIPS; k++) {
        const int e = k * kStudyThreads + (int)threadIdx.x;
        const int ty = e / ROW, tx = (e - ty * ROW) * V;
        if (!(ty < t.th && tx < t.tw)) continue;
        PixelChunk<V> v = loaded[k];
        for (int j = 0; j < m; j++) {   // m is the same in every lane; 0 in most tiles
            const Entry d = list[j];
            const int dy = ty - d.y;
            if (dy < -d.r || dy > d.r || tx + V - 1 < d.x - d.r || tx > d.x + d.r) continue;
            typename R::Row row = R::row(d, j, dy, tx, staged);
#pragma unroll
            for (int q = 0; q < V; q++) R::pixel(d, row, tx + q - d.x, v.px[q]);
        }
        *reinterpret_cast<Word*>(out + (size_t)(t.y0 + ty) * n + (t.x0 + tx)) = v.w;
    }
}

// What the launchers of the three kernels share: one workgroup per tile, the widest V
template <typename Launch>
inline void launch_insert(Launch&& launch, const uint16_t* src, uint16_t* out, int n) {
    const unsigned tiles = (unsigned)((n + kSimTile - 1) / kSimTile);
    launch_by_width([&](auto v) { launch(v, dim3(tiles * tiles), dim3(kStudyThreads)); }, n, src, out);
}

// Whether the square centre (x, y) +- r, in tile coordinates, meets the tile
__device__ __forceinline__ bool square_meets(int x, int y, int r, const TileGeom& t) { return !(x + r < 0 || x - r >= t.tw || y + r < 0 || y - r >= t.th); }

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

// n >= 1 consecutive bytes at p as one word, byte k in bits 8k: the first four when n >= 4 (one load), else the n of a ragged tail
__device__ __forceinline__ uint32_t load_bytes4(const GlobalU8* p, int n) {
    uint32_t word = 0u;
    if (n >= 4) {
        __builtin_memcpy(&word, p, 4);   // 1-byte aligned
        return word;
    }
    for (int k = 0; k < n; k++) word |= (uint32_t)p[k] << (8 * k);
    return word;
}

// A cols x rows window of both sides of a comparison as packed bytes in LDS, `pitch` words a row, `words` >= ceil(cols / 4) of them
// written in each of `lds_rows` rows: pixel x of a row in byte x & 3 of word x >> 2, every byte beyond the window 0. pa / pb: the
// window's first pixel. Side a is quantised on the way (load_quant4). Nothing outside the cols x rows pixels is read. The caller's
// barrier stands behind it.
__device__ __forceinline__ void stage_windows(const GlobalF32* __restrict__ pa, int a_pitch, const GlobalU8* __restrict__ pb, int b_pitch, int cols, int rows,
                                              uint32_t* __restrict__ wa, uint32_t* __restrict__ wb, int pitch, int words, int lds_rows) {
    for (int i = threadIdx.x; i < lds_rows * words; i += kStudyThreads) {
        const int r = i / words, wd = i - r * words, x = wd << 2;
        uint32_t a = 0u, b = 0u;
        if (r < rows && x < cols) {
            a = load_quant4(pa + (ptrdiff_t)r * a_pitch + x, cols - x);
            b = load_bytes4(pb + (ptrdiff_t)r * b_pitch + x, cols - x);
        }
        wa[r * pitch + wd] = a;
        wb[r * pitch + wd] = b;
    }
}

// stage_windows' loads by the side's pixel type: side a (graded f32, quantised on the way) or side b (bytes)
__device__ __forceinline__ uint32_t load_pixels4(const GlobalF32* p, int n) { return load_quant4(p, n); }
__device__ __forceinline__ uint32_t load_pixels4(const GlobalU8* p, int n) { return load_bytes4(p, n); }

// ONE side's window as packed bytes in LDS, `words` words in each of `lds_rows` rows of `pitch` words, where the window may hang over
// the pixels that may be read: window pixel (c, r) is region pixel (ox + c, oy + r), `p` the REGION's first pixel, and only the region
// pixels x_lo <= x < x_hi, y_lo <= y < y_hi (the caller's tile and its halo, clipped to the region) are read; every other byte of the
// staged words is 0. ox may be negative. map(word): what is stored of a word of four pixels (k_cooccurrence: their levels;
// k_granulometry: the bytes or their complements; k_contour_mask: the bytes). `outside`, where not 0: the word whose bytes stand behind map() for the pixels that
// were not read (k_granulometry: 255, the neutral value of an erosion). The caller's barrier stands behind it.
template <typename Px, typename Map>
__device__ __forceinline__ void stage_halo_window(const Px* __restrict__ p, int pitch_px, int ox, int oy, int x_lo, int x_hi, int y_lo, int y_hi,
                                                  uint32_t* __restrict__ win, int pitch, int words, int lds_rows, Map map, uint32_t outside = 0u) {
    for (int i = threadIdx.x; i < lds_rows * words; i += kStudyThreads) {
        const int r = i / words, wd = i - r * words;
        const int y = oy + r, x = ox + (wd << 2);
        uint32_t v = 0u, read = 0u;   // read: 0xFF in the bytes that were read
        if (y >= y_lo && y < y_hi) {
            const int lo = max(x, x_lo), hi = min(x + 4, x_hi);   // the word's pixels that may be read: all four, or a ragged end
            if (lo < hi) {
                v = load_pixels4(p + (ptrdiff_t)y * pitch_px + lo, hi - lo) << (8 * (lo - x));
                read = (0xFFFFFFFFu >> (8 * (4 - (hi - lo)))) << (8 * (lo - x));
            }
        }
        win[r * pitch + wd] = outside ? (map(v) & read) | (outside & ~read) : map(v);
    }
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
