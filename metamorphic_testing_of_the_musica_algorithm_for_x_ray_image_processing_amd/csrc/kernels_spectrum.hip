// kernels_spectrum.hip — the spectrum metric of the study (musica_sim_spectrum, include/musica.h; metrics.spectrum_statistics): the exact
// Walsh-Hadamard transforms of a comparison. A region holds (w / T) x (h / T) whole tiles of T x T pixels, T in {8, 16, 32, 64}, anchored at
// its first pixel on either side; per tile A = W a W^T and B = W b W^T in integers (W the T x T Walsh matrix in sequency order), and per
// coefficient [sv][su] the three exact sums over the tiles: A^2, B^2, A B (signed). Side a is the graded f32 plane of a batch image
// quantised with out_u8 while it is read (load_quant4: exactly what k_sim and k_lattice read), side b a reference slot. No float anywhere.
//
// k_spectrum<T>: a query owns blockIdx.z and `groups` PERSISTENT workgroups of kStudyThreads threads; workgroup g takes the 64 x 64
// blocks g, g + groups, .. of the query's tiled area, (w / T) T x (h / T) T pixels (tile_geom). A block holds (64 / T)^2 tiles; a ragged
// last block holds fewer, and because the tiled area is whole tiles and stage_windows writes zeros beyond it, the tiles of a block that
// lie outside are all zero on both sides: their coefficients are 0 and they add nothing, with no test in the arithmetic.
//   stage    both 64 x 64 windows once, as packed bytes in LDS (stage_windows, 16 words a row): 4 + 1 bytes a pixel from memory, once.
//   rows     thread t takes the 16 consecutive pixels 16 q .. 16 q + 15 (q = t & 3) of row t / 4: one ds_read_b128 a side. The butterflies
//            (x, y) -> (x + y, x - y) of the column bits 0 .. 3 are adds and subtracts between its 16 registers; bits 4 and 5 pair the
//            four neighbouring lanes of a row, read by DPP quad_perm [1, 0, 3, 2] and [2, 3, 0, 1]: the lane whose bit is clear keeps
//            x + y, the other one x - y, its partner's value minus its own (spectrum_pass). The stages of bits >= log2 T are compiled out: the tiles of a row transform side by side.
//   turn     the row coefficients go through one int32 plane a side in LDS and come back with thread t holding the rows 16 q .. 16 q + 15 of
//            column t / 4. Banks of ds_write_b32 / ds_read_b32 are word % 32 over the two halves of a wavefront; a half is 8 rows (columns)
//            x 4 chunks that start 16 apart, so a pitch of 65 would put the chunks q and q + 2 on one bank. The plane's word of (row, x) is
//            row * 73 + 8 (row >> 5) + x + 8 (x >> 5): 73 = 9 (mod 32) keeps 8 neighbouring rows apart mod 8, and the skews move the
//            chunks to 0, 16, 8 + 32, 24 + 32 (mod 32: 0, 16, 8, 24): all 32 lanes of a half on their own bank, written and read.
//   columns  the same butterflies down the column. A thread then holds 16 coefficients of A and of B at the same positions of the
//            block, in NATURAL (Hadamard) order: position (v, u) is coefficient (v mod T, u mod T) of tile (v / T, u / T).
//   sums     A^2, B^2 and A B into 48 64-bit REGISTER accumulators, one 32 x 32 -> 64 multiply-add each, kept over all its blocks:
//            neither LDS nor memory is touched per coefficient.
//   flush    once a workgroup, behind its last block: per word, the accumulators of the positions congruent mod T meet in an LDS table
//            of T x T u64 in the (now free) planes, by LDS atomics ((64 / T)^2 adds a word; plain stores at T = 64, where a position is a
//            coefficient), and the workgroup stores the T x T words as its own partial table [word][v][u]: plain coalesced stores, zeros
//            included. A partial table is 3 T^2 words: 1.5 KiB at T = 8, 96 KiB at T = 64.
// k_spectrum_fold: a thread takes a word of the partial tables and one of kSpectrumFoldSlices slices of the query's workgroups, sums them
// (coalesced reads), maps the natural indices to sequencies (spectrum_sequency: Gray decoding of the reversed bits, asserted below against
// the sign changes of the Sylvester rows) and adds the sum to the query's table, which the caller zeroes on the stream, with one 64-bit
// integer global atomic. Integer sums commute, two's complement included: exact and byte-identical from call to call.
// THE 64-BIT RULE. |A|, |B| <= 255 T^2 < 2^20, so a tile adds at most 2^40 to a word; a region side is below 2^14 (16364), which gives at
// most 2^16 tiles at T = 64 (2^56) and at most 2^22 tiles of at most 2^28 at T = 8 (2^50): below 2^63 in every accumulator, partial and sum.
#include "study_device.h"

namespace musica {

constexpr int kSpectrumWinWords = kSimTile / 4;                    // words of a staged window row
constexpr int kSpectrumPitch = 73;                                 // words between the rows of a turning plane
constexpr int kSpectrumPlaneWords = kSimTile * kSpectrumPitch + 16; // both skews of the last row behind it
constexpr int kSpectrumFoldSlices = 16;
static_assert(kSimTile == 64 && kStudyThreads == 256 && kSpectrumWinWords == 16, "a thread takes 16 pixels of a row: four lanes a row, 64 rows");
static_assert(kSpectrumPitch >= kSimTile + 8 && kSpectrumPitch % 8 == 1, "a row and its skew fit in the pitch; 8 neighbouring rows differ mod 8");
static_assert(2 * kSpectrumPlaneWords * sizeof(int32_t) >= (size_t)kSimTile * kSimTile * sizeof(unsigned long long), "the flush table of one word lies in the two planes");
static_assert(kSpectrumWords == 3, "A^2, B^2, A B");

// The sequency of row n of the Sylvester Hadamard matrix of order T: reverse the log2 T bits, then decode the Gray code.
constexpr int spectrum_sequency(int n, int T) {
    int r = 0;
    for (int bit = 1, back = T >> 1; bit < T; bit <<= 1, back >>= 1)
        if (n & bit) r |= back;
    int s = 0;
    for (; r; r >>= 1) s ^= r;
    return s;
}
// The sign changes of that row, counted: H[n][x] = (-1)^popcount(n & x)
constexpr int spectrum_sign_changes(int n, int T) {
    int changes = 0;
    for (int x = 1; x < T; x++) changes += (__builtin_popcount(n & x) ^ __builtin_popcount(n & (x - 1))) & 1;
    return changes;
}
constexpr bool spectrum_sequencies_hold(int T) {
    for (int n = 0; n < T; n++)
        if (spectrum_sequency(n, T) != spectrum_sign_changes(n, T)) return false;
    return true;
}
static_assert(spectrum_sequencies_hold(8) && spectrum_sequencies_hold(16) && spectrum_sequencies_hold(32) && spectrum_sequencies_hold(64),
              "spectrum_sequency is the number of sign changes of the Sylvester row");

template <int T>
struct SpectrumOrder {
    int seq[T];
    constexpr SpectrumOrder() : seq() {
        for (int n = 0; n < T; n++) seq[n] = spectrum_sequency(n, T);
    }
};

template <int CTRL>
__device__ __forceinline__ int spectrum_quad(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);   // quad_perm: every lane has a source
}

// The Walsh-Hadamard butterflies of 64 values, 16 in each of the four lanes of a quad (value 16 q + k is v[k] of lane q), over the index
// bits below log2 T, in place and in natural order. odd4 / odd5: bit 0 / bit 1 of the lane's q: such a lane takes its partner's value
// minus its own, the other one the sum. Compiled, a lane stage is a negation, a select and an add with a DPP operand; (own ^ m) + (partner - m) with m = 0 / -1 came out as
// three operations as well (v_xor, v_mov_dpp, v_add3).
template <int T>
__device__ __forceinline__ void spectrum_pass(int (&v)[16], bool odd4, bool odd5) {
#pragma unroll
    for (int s = 1; s < 16 && s < T; s <<= 1)
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (!(i & s)) {
                const int x = v[i], y = v[i | s];
                v[i] = x + y;
                v[i | s] = x - y;
            }
    if (T > 16) {
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = spectrum_quad<0xB1>(v[i]) + (odd4 ? -v[i] : v[i]);   // quad_perm:[1,0,3,2]
    }
    if (T > 32) {
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = spectrum_quad<0x4E>(v[i]) + (odd5 ? -v[i] : v[i]);   // quad_perm:[2,3,0,1]
    }
}

// The 16 pixels of a thread from its four window words
__device__ __forceinline__ void spectrum_unpack(const uint4 w, int (&v)[16]) {
    const uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = (int)((word[i >> 2] >> (8 * (i & 3))) & 0xFFu);
}

// Where (row, x) of a turning plane lies
__device__ __forceinline__ int spectrum_word(int row, int x) { return row * kSpectrumPitch + 8 * (row >> 5) + x + 8 * (x >> 5); }

template <int T>
__global__ __launch_bounds__(kStudyThreads) void k_spectrum(const SpectrumQueryDev* __restrict__ qs, unsigned long long* __restrict__ part) {
    constexpr int COEFFS = T * T;
    __shared__ __attribute__((aligned(16))) uint32_t wa[kSimTile * kSpectrumWinWords], wb[kSimTile * kSpectrumWinWords];
    __shared__ __attribute__((aligned(16))) int32_t plane[2 * kSpectrumPlaneWords];
    const SpectrumQueryDev q = qs[blockIdx.z];
    if ((int)blockIdx.x >= q.groups) return;   // whole workgroup: the grid is sized for the query with the most groups
    const int t = threadIdx.x, lane_q = t & 3, line = t >> 2;   // row `line` of the row pass, column `line` of the column pass
    const bool odd4 = lane_q & 1, odd5 = lane_q & 2;
    int32_t* const pa = plane;
    int32_t* const pb = plane + kSpectrumPlaneWords;
    const int put = spectrum_word(line, 16 * lane_q);   // + k: 16 neighbouring words, inside one half of the row
    const int get = spectrum_word(16 * lane_q, line);   // + k * kSpectrumPitch: 16 neighbouring rows, inside one half of the plane

    long long acc[kSpectrumWords][16];
#pragma unroll
    for (int f = 0; f < kSpectrumWords; f++)
#pragma unroll
        for (int k = 0; k < 16; k++) acc[f][k] = 0;

    const int blocks = q.tiles_x * q.tiles_y;
    for (int block = blockIdx.x; block < blocks; block += q.groups) {
        const TileGeom g = tile_geom(block, q.tiles_x, q.tiled_w, q.tiled_h);
        __syncthreads();   // the last block's windows and planes are read
        stage_windows((const GlobalF32*)q.a + (ptrdiff_t)g.y0 * q.a_pitch + g.x0, q.a_pitch, (const GlobalU8*)q.b + (ptrdiff_t)g.y0 * q.b_pitch + g.x0, q.b_pitch,
                      g.tw, g.th, wa, wb, kSpectrumWinWords, kSpectrumWinWords, kSimTile);
        __syncthreads();
        int a[16], b[16];
        spectrum_unpack(*reinterpret_cast<const uint4*>(wa + line * kSpectrumWinWords + 4 * lane_q), a);
        spectrum_pass<T>(a, odd4, odd5);
#pragma unroll
        for (int k = 0; k < 16; k++) pa[put + k] = a[k];
        spectrum_unpack(*reinterpret_cast<const uint4*>(wb + line * kSpectrumWinWords + 4 * lane_q), b);
        spectrum_pass<T>(b, odd4, odd5);
#pragma unroll
        for (int k = 0; k < 16; k++) pb[put + k] = b[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; k++) a[k] = pa[get + k * kSpectrumPitch];
        spectrum_pass<T>(a, odd4, odd5);
#pragma unroll
        for (int k = 0; k < 16; k++) b[k] = pb[get + k * kSpectrumPitch];
        spectrum_pass<T>(b, odd4, odd5);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            acc[0][k] += (long long)a[k] * a[k];
            acc[1][k] += (long long)b[k] * b[k];
            acc[2][k] += (long long)a[k] * b[k];
        }
    }

    // position (16 lane_q + k, line) of the block is coefficient (v mod T, u mod T): one word at a time through a T x T table in the planes
    unsigned long long* const tab = reinterpret_cast<unsigned long long*>(plane);
    GlobalU64* const mine = (GlobalU64*)part + q.part + (size_t)blockIdx.x * (kSpectrumWords * COEFFS);   // blockIdx.x < q.groups: inside the query's partials
    const int at = ((16 * lane_q) & (T - 1)) * T + (line & (T - 1));
#pragma unroll
    for (int f = 0; f < kSpectrumWords; f++) {
        __syncthreads();   // the planes, or the last word's table, are read
        if (T < kSimTile) {
            for (int i = t; i < COEFFS; i += kStudyThreads) tab[i] = 0ull;
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int i = at + (k & (T - 1)) * T;   // 16 lane_q is a multiple of 16 and k < 16: they add without a carry, so (16 lane_q + k) mod T is the sum of the two masked
            if (T < kSimTile) atomicAdd(&tab[i], (unsigned long long)acc[f][k]);
            else tab[i] = (unsigned long long)acc[f][k];
        }
        __syncthreads();
        for (int i = t; i < COEFFS; i += kStudyThreads) mine[f * COEFFS + i] = tab[i];
    }
}

// Word i = (word * T + v) * T + u of the partial tables slice, slice + kSpectrumFoldSlices, .. of a query (blockIdx.y: the slice), summed
// and added to word (seq(v) * T + seq(u)) * 3 + word of its table. Eight loads in flight a thread, as k_lattice_fold.
template <int T>
__global__ __launch_bounds__(kStudyThreads) void k_spectrum_fold(const SpectrumQueryDev* __restrict__ qs, const unsigned long long* __restrict__ part,
                                                                  unsigned long long* __restrict__ tables) {
    constexpr SpectrumOrder<T> order;
    constexpr int COEFFS = T * T, WORDS = kSpectrumWords * COEFFS;
    const SpectrumQueryDev q = qs[blockIdx.z];
    const int i = (int)(blockIdx.x * kStudyThreads + threadIdx.x);
    if (i >= WORDS) return;
    const GlobalU64* p = (const GlobalU64*)part + q.part + i;
    unsigned long long sum = 0ull;
    int g = (int)blockIdx.y;
    for (; g + 7 * kSpectrumFoldSlices < q.groups; g += 8 * kSpectrumFoldSlices) {
        unsigned long long v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = p[(size_t)(g + k * kSpectrumFoldSlices) * WORDS];
#pragma unroll
        for (int k = 0; k < 8; k++) sum += v[k];
    }
    for (; g < q.groups; g += kSpectrumFoldSlices) sum += p[(size_t)g * WORDS];
    const int f = i / COEFFS, c = i - f * COEFFS, v = c / T, u = c - v * T;
    if (sum) atomicAdd((unsigned long long*)((GlobalU64*)tables + q.table + (size_t)(order.seq[v] * T + order.seq[u]) * kSpectrumWords + f), sum);
}

template <int T>
static void launch_spectrum(hipStream_t st, const SpectrumQueryDev* d_qs, int count, int max_groups, unsigned long long* part, unsigned long long* tables) {
    const dim3 block(kStudyThreads);
    hipLaunchKernelGGL(k_spectrum<T>, dim3((unsigned)max_groups, 1, (unsigned)count), block, 0, st, d_qs, part);
    constexpr int WORDS = kSpectrumWords * T * T;
    hipLaunchKernelGGL(k_spectrum_fold<T>, dim3((unsigned)((WORDS + kStudyThreads - 1) / kStudyThreads), kSpectrumFoldSlices, (unsigned)count), block, 0, st, d_qs, part, tables);
}

void launch_sim_spectrum(hipStream_t st, const SpectrumQueryDev* d_qs, int count, int max_groups, int tile, unsigned long long* part, unsigned long long* tables) {
    switch (tile) {
        case 8: launch_spectrum<8>(st, d_qs, count, max_groups, part, tables); break;
        case 16: launch_spectrum<16>(st, d_qs, count, max_groups, part, tables); break;
        case 32: launch_spectrum<32>(st, d_qs, count, max_groups, part, tables); break;
        case 64: launch_spectrum<64>(st, d_qs, count, max_groups, part, tables); break;
        default: return;
    }
}

}  // namespace musica
