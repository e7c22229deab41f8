// kernels_gratings.hip — the grating relation of the study (include/musica.h, musica_alter_gratings / musica_sim_gratings): sine (or any)
// wave patches inserted into the alteration source on its way into one image of the input buffer, and the phase-folded tables of an
// output against a reference slot. A grating is (x, y, h, ux, uy, T) plus a wave table of T int16: an integer centre, a half-side
// kGratingMinHalf <= h <= kGratingMaxHalf, a wave vector (ux, uy) with |ux|, |uy| <= kGratingMaxU, not both 0, gcd(|ux|, |uy|) = 1, a
// period 2 <= T <= kGratingMaxPeriod with T <= h, 2|ux| <= T and 2|uy| <= T. With dx = px - x, dy = py - y the phase of a pixel is
// k = (ux dx + uy dy) mod T in 0 .. T - 1. The plate |dx|, |dy| <= 2h (side 4h + 1) is inserted, the region |dx|, |dy| <= h (side
// S = 2h + 1) measured. The plates of a list lie inside the plane and are pairwise disjoint (the callers check), so a pixel belongs to
// at most one plate. A list travels packed, PackedGrating (launchers.h): a plane side is at most 16384.
//
// k_alter_gratings<V>: harness.insert_gratings, the insertion body of study_device.h (insert_patches: bin, stage, stream) with the rule:
// inside a plate
//   out = min((v (1024 - wave[k]) + 512) >> 10, 65535)      |wave| <= 512: v (1024 - wave) + 512 <= 65535 * 1536 + 512 < 2^32, exact u32,
//                                                            ONE rounding (asserted below on the limits); wave = 0 gives v
// The listed square of a grating is its plate.
//   CAPACITY k_alter_edges' argument: a plate has side 4h + 1 >= 33, so along an axis a listed plate covers at least 33 of the
//            128 positions -32 .. 95 of the tile grown by 32; the plates are disjoint and each holds at least 33^2 = 1089 of those
//            128^2 = 16384 pixels: at most floor(16384 / 1089) = 15 are listed.
//   stage    the listed gratings' wave tables are staged next to the list, T <= 64 int16 each: at most 15 x 64 x 2 B = 1920 B.
//   row      a chunk that meets a plate takes the phase of its first pixel with one remainder and carries it along the chunk as
//            k += ux with one wrap (|ux| < T): no division per pixel for V = 8 and 2. (V = 1, the fallback for odd sides, has
//            one-pixel chunks and so takes the remainder per plate pixel.)
// 2.3 KB of LDS. Beyond the two planes only the list's waves are read.
//
// k_sim_gratings: harness.grating_statistics. One workgroup of 256 threads per grating; side a is the graded f32 plane of a batch image
// quantised with out_u8 while it is read (exactly what k_sim reads), side b the slot's u8 plane, the grating in the coordinates of the
// cropped output plane. Every pixel of the region adds 1, a, b and a^2 into bin k of the grating's [4][T] table.
//   TWO FACTS (tests/test_grating_restatement.py holds both over every admissible (ux, uy, T)):
//     every bin is non-empty   dx and dy each run over S >= 2T + 1 consecutive values, so ux dx reaches every multiple of gcd(ux, T)
//            mod T and uy dy every multiple of gcd(uy, T); their sums reach every multiple of gcd(ux, uy, T) = 1.
//     a bin holds at most ceil(S / 2) S pixels   one of ux, uy is not 0 mod T (2|u| <= T makes |u| < T, and both 0 would make them
//            both 0, gcd 1 forbids), so along that axis the same phase repeats with a period of at least 2: at most ceil(S / 2)
//            pixels of each of the S lines along it. S <= 257: 129 * 257 = 33153 pixels, 33153 * 255^2 < 2^32 (asserted below).
//   WHY NOT ONE LDS ATOMIC PER PIXEL. The table has T <= 64 words a row: in a row of the region every T / gcd(ux, T)-th lane of a
//            wavefront adds to the same word, all 64 for ux = 0, and the LDS serialises them (k_sim_edges spreads a row over hundreds of
//            bins and meets 5-fold collisions at most). So the sums are taken in registers ALONG THE BARS, where the phase does not
//            change, and added to LDS once per bar (ds_add_u32, no return; integer addition commutes, so the table is exact and
//            repeats from call to call whatever order the wavefronts arrive in). MEASURED (the 81-grating phantom of
//            3072^2): 27.2 us against 28.3 us for a build with the atomics per pixel, inside one another's spread: at that phantom the
//            kernel is bound by the serial walk of its largest regions over cold planes, not by the LDS. The walk is kept because it
//            is no slower and its LDS traffic does not depend on T or on the direction.
//   walk, ux != 0   the phase is constant along the lattice direction v = (-uy, ux) sign(ux), vy = |ux| >= 1. A STRAND (r, c), 0 <= r <
//            vy, 0 <= c < S, visits the pixels ((c + j vx) mod S, r + j vy), j = 0, 1 .. while the row is inside: the lines of
//            direction v through row r, joined end to start by the wrap of x. Every pixel (x, y) lies on exactly one strand, r = y mod
//            vy and c = (x - (y div vy) vx) mod S, at exactly one j. Threads take the vy S <= 2056 strands round-robin, so the lanes of
//            a wavefront hold consecutive c of one r (or the end of one r and the start of the next) and every step reads a run of
//            consecutive pixels of one row, in at most two pieces: coalesced, which lines started from a COLUMN of the region would not
//            be. Between two wraps a strand is one bar: n, sum a, sum b, sum a^2 are summed in registers (at most S pixels) and
//            flushed to bin k at a wrap and at the end; the wrap moves k by -+ (ux S mod T), one conditional add. A strand has
//            ceil((S - r) / vy) pixels and at most |uy| + 1 flushes. kGratingSteps steps are loaded together, since the walk is bound
//            by the latency of its loads. One remainder per strand, no division per pixel.
//   walk, ux = 0    then uy = +-1 and a row has ONE phase, (uy dy) mod T. The wavefronts take the rows round-robin, the lanes the columns
//            in steps of 64; the row's four sums go through wave_sum and the wavefront's leader adds them once.
//   roi_ssd  u32 per lane (asserted below for every |ux|), then the study's ONE reduction order (wave_sum, then WaveSlots).
// After a barrier the workgroup writes the table's 4 T words to its place in the flat output and thread 0 the four u64 of the result.
// No global atomics, integer only.
#include "study_device.h"

namespace musica {

constexpr int kGratingThreads = 256;
constexpr int kGratingTileCap = 15;   // listed plates of one tile: CAPACITY above
constexpr int kGratingMinPlate = 4 * kGratingMinHalf + 1;
constexpr int kGratingSteps = 4;      // steps of a strand (rows of a column, ux = 0) that a lane loads together
constexpr int kGratingSide = 2 * kGratingMaxHalf + 1;
static_assert(kGratingThreads == kStudyThreads, "k_sim_gratings reduces over the study's workgroup");
static_assert(kGratingMinPlate == 33 && ((kSimTile + 2 * (kGratingMinPlate - 1)) * (kSimTile + 2 * (kGratingMinPlate - 1))) / (kGratingMinPlate * kGratingMinPlate) == kGratingTileCap,
              "the capacity argument: plates of side >= 33 in the tile grown by 32");
static_assert(65535ull * (1024ull + kGratingMaxContrast) + 512ull < (1ull << 32), "the attenuated pixel is an exact u32");
static_assert(kGratingMaxContrast <= 1024, "1024 - wave >= 0");
static_assert(kGratingMaxPeriod <= 64 && 2 * kGratingMaxU <= kGratingMaxPeriod, "a wave fits its LDS row; |u| < T: one wrap a step");
static_assert(((kGratingSide + 1ull) / 2) * kGratingSide * 255 * 255 < (1ull << 32), "a bin's sums fit u32: at most ceil(S / 2) S pixels");
static_assert(kGratingMaxHalf < 256 && kGratingMaxPeriod < 256 && kGratingMaxU < 128, "a grating packs into PackedGrating");

// the most pixels a lane of k_sim_gratings sums into its u32 roi_ssd: its strands times a strand's steps, for every vy = |ux|; the
// rows of a wavefront times a lane's columns for ux = 0
constexpr unsigned long long grating_lane_pixels() {
    unsigned long long most = (unsigned long long)((kGratingSide + kStudyWaves - 1) / kStudyWaves) * ((kGratingSide + 63) / 64);
    for (int vy = 1; vy <= kGratingMaxU; vy++) {
        const unsigned long long strands = (unsigned long long)(vy * kGratingSide + kGratingThreads - 1) / kGratingThreads, steps = (kGratingSide + vy - 1) / vy;
        most = strands * steps > most ? strands * steps : most;
    }
    return most;
}
static_assert(grating_lane_pixels() * 255ull * 255ull < (1ull << 32), "a lane's roi_ssd over the largest region fits u32");

__device__ __forceinline__ int grating_ux(uint32_t htuv) { return (int)(int8_t)((htuv >> 16) & 0xFFu); }
__device__ __forceinline__ int grating_uy(uint32_t htuv) { return (int)(int8_t)(htuv >> 24); }

// t mod q in 0 .. q - 1 for q > 0 and any t
__device__ __forceinline__ int floor_mod(int t, int q) {
    const int m = t % q;
    return m < 0 ? m + q : m;
}

struct GratingInsert {
    typedef PackedGrating Packed;
    struct Entry {
        int x, y, r, ux, uy, t;   // centre in tile coordinates, the plate's reach 2h, the wave vector, the period
        uint32_t first;           // where its wave begins in the list's waves
    };
    typedef int16_t Wave[kGratingMaxPeriod];
    struct Staged {
        const Wave* wave;         // the listed gratings' waves, in LDS
    };
    struct Row {
        const int16_t* wave;
        int phase;                // of the next pixel of the chunk
    };
    static constexpr int kTileCap = kGratingTileCap;
    static __device__ __forceinline__ bool meets(const PackedGrating& g, const TileGeom& t, Entry& e) {
        e = {(int)(g.xy & 0xFFFFu) - t.x0, (int)(g.xy >> 16) - t.y0, 2 * (int)(g.htuv & 0xFFu), grating_ux(g.htuv), grating_uy(g.htuv),
             (int)((g.htuv >> 8) & 0xFFu), g.first};
        return square_meets(e.x, e.y, e.r, t);
    }
    static __device__ __forceinline__ Staged stage(const Entry* list, int m, const int16_t* __restrict__ waves) {
        __shared__ Wave wave[kGratingTileCap];
        for (int i = threadIdx.x; i < m * kGratingMaxPeriod; i += kGratingThreads) {   // nothing in most tiles
            const int j = i / kGratingMaxPeriod, k = i - j * kGratingMaxPeriod;
            if (k < list[j].t) wave[j][k] = waves[list[j].first + k];
        }
        __syncthreads();
        return {wave};
    }
    static __device__ __forceinline__ Row row(const Entry& d, int j, int dy, int tx, const Staged& s) {
        return {s.wave[j], floor_mod(d.ux * (tx - d.x) + d.uy * dy, d.t)};
    }
    static __device__ __forceinline__ void pixel(const Entry& d, Row& row, int dx, uint16_t& px) {
        if (dx >= -d.r && dx <= d.r) px = (uint16_t)min(((uint32_t)px * (uint32_t)(1024 - (int)row.wave[row.phase]) + 512u) >> 10, 65535u);
        row.phase += d.ux;
        row.phase = row.phase >= d.t ? row.phase - d.t : row.phase < 0 ? row.phase + d.t : row.phase;
    }
};

// n % V == 0 and both planes aligned to 2 V bytes
template <int V>
__global__ __launch_bounds__(kGratingThreads) void k_alter_gratings(const uint16_t* __restrict__ src, uint16_t* __restrict__ out, int n,
                                                                     const PackedGrating* __restrict__ gratings, const int16_t* __restrict__ waves, int count) {
    insert_patches<GratingInsert, V>(src, out, n, gratings, count, waves);
}

void launch_alter_gratings(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const PackedGrating* d_gratings, const int16_t* d_waves, int count) {
    launch_insert([&](auto v, dim3 grid, dim3 block) { hipLaunchKernelGGL((k_alter_gratings<decltype(v)::value>), grid, block, 0, st, src, out, n, d_gratings, d_waves, count); },
                  src, out, n);
}

// a: the graded f32 plane at output pixel (0, 0) (the margin skipped), b: the slot's plane; results: count x kGratingWords u64; tables:
// grating i's 4 x T_i u32 at 4 * PackedGrating::first
__global__ __launch_bounds__(kGratingThreads) void k_sim_gratings(const float* __restrict__ a_plane, int a_pitch, const uint8_t* __restrict__ b_plane,
                                                                   int b_pitch, const PackedGrating* __restrict__ gratings,
                                                                   unsigned long long* __restrict__ results, uint32_t* __restrict__ tables) {
    __shared__ uint32_t table[4][kGratingMaxPeriod];
    __shared__ WaveSlots<unsigned long long> slots;
    const PackedGrating g = gratings[blockIdx.x];
    const int h = (int)(g.htuv & 0xFFu), period = (int)((g.htuv >> 8) & 0xFFu), ux = grating_ux(g.htuv), uy = grating_uy(g.htuv);
    const int side = 2 * h + 1;
    // the region's pixel (0, 0)
    const GlobalF32* pa = (const GlobalF32*)a_plane + (size_t)((int)(g.xy >> 16) - h) * a_pitch + ((int)(g.xy & 0xFFFFu) - h);
    const GlobalU8* pb = (const GlobalU8*)b_plane + (size_t)((int)(g.xy >> 16) - h) * b_pitch + ((int)(g.xy & 0xFFFFu) - h);
    if (threadIdx.x < 4 * kGratingMaxPeriod) (&table[0][0])[threadIdx.x] = 0u;
    __syncthreads();

    uint32_t ssd = 0u;
    if (ux != 0) {
        const int vy = ux > 0 ? ux : -ux, vx = ux > 0 ? -uy : uy;
        const int turn = floor_mod(ux * side, period);   // what a wrap of x by the side moves the phase by
        const int strands = vy * side;
        for (int s = threadIdx.x; s < strands; s += kGratingThreads) {
            const int r = s / side, c = s - r * side;
            int x = c, k = floor_mod(ux * (c - h) + uy * (r - h), period);
            uint32_t cnt = 0u, sa = 0u, sb = 0u, saa = 0u;
            for (int y = r; y < side; y += kGratingSteps * vy) {
                uint32_t a[kGratingSteps], b[kGratingSteps];
                int xx = x;
                // a step past the region is loaded in the region's last row and counted nowhere
#pragma unroll
                for (int j = 0; j < kGratingSteps; j++) {
                    const int yy = min(y + j * vy, side - 1);
                    a[j] = out_u8(pa[(size_t)yy * a_pitch + xx]);
                    b[j] = pb[(size_t)yy * b_pitch + xx];
                    xx += vx;
                    xx = xx >= side ? xx - side : xx < 0 ? xx + side : xx;
                }
#pragma unroll
                for (int j = 0; j < kGratingSteps; j++) {
                    if (y + j * vy < side) {
                        const uint32_t diff = a[j] > b[j] ? a[j] - b[j] : b[j] - a[j];
                        ssd += diff * diff;
                        cnt++;
                        sa += a[j];
                        sb += b[j];
                        saa += a[j] * a[j];
                    }
                    x += vx;
                    if (x >= side || x < 0) {   // the bar ends here: its sums go to its bin, the next bar's phase is `turn` away
                        if (cnt && (unsigned)k < (unsigned)period) {
                            atomicAdd(&table[0][k], cnt);
                            atomicAdd(&table[1][k], sa);
                            atomicAdd(&table[2][k], sb);
                            atomicAdd(&table[3][k], saa);
                        }
                        cnt = sa = sb = saa = 0u;
                        if (x >= side) {
                            x -= side;
                            k -= turn;
                            k = k < 0 ? k + period : k;
                        } else {
                            x += side;
                            k += turn;
                            k = k >= period ? k - period : k;
                        }
                    }
                }
            }
            if (cnt && (unsigned)k < (unsigned)period) {
                atomicAdd(&table[0][k], cnt);
                atomicAdd(&table[1][k], sa);
                atomicAdd(&table[2][k], sb);
                atomicAdd(&table[3][k], saa);
            }
        }
    } else {
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int row0 = wave; row0 < side; row0 += kStudyWaves * kGratingSteps) {
            uint32_t cnt[kGratingSteps], sa[kGratingSteps], sb[kGratingSteps], saa[kGratingSteps];
#pragma unroll
            for (int j = 0; j < kGratingSteps; j++) cnt[j] = sa[j] = sb[j] = saa[j] = 0u;
            for (int col = lane; col < side; col += 64) {
                uint32_t a[kGratingSteps], b[kGratingSteps];
#pragma unroll
                for (int j = 0; j < kGratingSteps; j++) {
                    const int yy = min(row0 + j * kStudyWaves, side - 1);
                    a[j] = out_u8(pa[(size_t)yy * a_pitch + col]);
                    b[j] = pb[(size_t)yy * b_pitch + col];
                }
#pragma unroll
                for (int j = 0; j < kGratingSteps; j++) {
                    const uint32_t diff = a[j] > b[j] ? a[j] - b[j] : b[j] - a[j];
                    if (row0 + j * kStudyWaves < side) ssd += diff * diff;
                    cnt[j]++;
                    sa[j] += a[j];
                    sb[j] += b[j];
                    saa[j] += a[j] * a[j];
                }
            }
#pragma unroll
            for (int j = 0; j < kGratingSteps; j++) {
                wave_sum(cnt[j], sa[j], sb[j], saa[j]);
                const int row = row0 + j * kStudyWaves;   // the same in every lane of the wavefront
                if (wave_leader() && row < side) {
                    const int k = floor_mod(uy * (row - h), period);
                    atomicAdd(&table[0][k], cnt[j]);
                    atomicAdd(&table[1][k], sa[j]);
                    atomicAdd(&table[2][k], sb[j]);
                    atomicAdd(&table[3][k], saa[j]);
                }
            }
        }
    }
    unsigned long long w = ssd;
    wave_sum(w);
    if (wave_leader()) slots.put(w);
    __syncthreads();   // the table is complete, the wavefronts' sums are in place
    uint32_t* o = tables + 4 * (size_t)g.first;
    if ((int)threadIdx.x < 4 * period) o[threadIdx.x] = table[threadIdx.x / period][threadIdx.x % period];
    if (threadIdx.x == 0) {
        // musica_sim_grating_result: roi_ssd, roi_pixels, table_offset, bins
        unsigned long long* r = results + (size_t)blockIdx.x * kGratingWords;
        r[0] = slots.sum();
        r[1] = (unsigned long long)side * side;
        r[2] = 4ull * g.first;
        r[3] = (unsigned long long)period;
    }
}

void launch_sim_gratings(hipStream_t st, const float* a_plane, int a_pitch, const uint8_t* b_plane, int b_pitch, const PackedGrating* d_gratings, int count,
                         unsigned long long* results, uint32_t* tables) {
    hipLaunchKernelGGL(k_sim_gratings, dim3((unsigned)count), dim3(kGratingThreads), 0, st, a_plane, a_pitch, b_plane, b_pitch, d_gratings, results, tables);
}

}  // namespace musica
