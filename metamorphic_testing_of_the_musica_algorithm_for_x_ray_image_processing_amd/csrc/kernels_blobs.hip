// kernels_blobs.hip — the cluster metric of the study (musica_sim_blobs, include/musica.h; metrics.blob_statistics): connected-component
// labelling of a comparison's change mask |a - b| > threshold, 4- or 8-connected, and per component its pixel count n, sum |a - b|,
// sum (a - b)^2 and bounding box, folded into a table by the class bit_length(n) - 1. Side a is the graded f32 plane of a batch image
// quantised with out_u8 while it is read (exactly what k_sim reads), side b a reference slot. Everything is an integer and the partition
// is unique: the tables, the largest component and the label planes equal the restatement word for word, whatever the interleaving.
//
// A pixel of a w x h region is named by its row-major index i = y w + x. The u32 plane `parent` holds, for a mask pixel, the index of
// another mask pixel of its component that is NOT LARGER than its own (kBlobNone off the mask): a forest whose roots are parent[i] == i.
// Every link that is ever written points to a smaller index, so a walk towards the root strictly descends, ends after fewer steps than
// the region has pixels, and the root of a finished component is its smallest index: its first pixel in row-major order, the canonical
// label. Five phases, each a launch of its own, so that no workgroup ever waits for another (no flag, no grid barrier, no spin):
//
//   k_blobs_tile<CONN>  a workgroup of kStudyThreads threads per 64 x 64 tile. Lane l of wavefront v reads column l of the rows v, v + 4, ..
//       (4 + 1 bytes a pixel, once); a row's mask is the wavefront's ballot, one 64-bit word a tile row in LDS. The tile is labelled
//       by a union-find over its RUNS (maximal horizontal stretches of mask pixels, at most 32 a row: id = 32 row + the run's ordinal,
//       which ascends with the row-major order of the runs' first pixels). Runs and their links to the row above come from bit
//       operations on the two row words: the starts are m & ~(m << 1), a run's ordinal a popcount, its first column a count of leading
//       zeros; a run meets a run of the row above where m & up has a bit (for 8: also where only up << 1 or up >> 1 has one), and of the
//       columns in which two runs overlap only the first unites them. union: find both roots, atomicMin the smaller into the larger
//       root's word (LDS), go on from what was there if it was no root any more. Then a run's last lane adds the run to its root's
//       record in LDS (n, sum |d|, sum d^2 from the wavefront's inclusive DPP scan of the row; x0, x1, y1 by atomicMin / atomicMax; y0
//       is the root's row): u32, 4096 * 255^2 fits. Every mask pixel's word of `parent` becomes the index of its tile-local root's
//       first pixel. A tile-local component that touches no side of its tile is a component of the region: it goes to the class table
//       (LDS, then one u64 atomic a non-zero word and tile) and competes for the tile's largest at once. One that touches a side (at
//       most 252 a tile: one border pixel each at least) gets a BlobRecord in the tile's block and its slot in the u32 plane `slots`
//       at its first pixel.
//   k_blobs_seam<CONN>  a thread per pixel of a tile's last column and last row: the pairs across the seam to the right and down and,
//       for 8, the diagonals across either (the single diagonal pairs of a four-tile corner among them). A pair is skipped where a
//       neighbouring pair provably unites the same two components. union on `parent` with atomicMin, as above.
//   k_blobs_flush       a thread per record: the final root of its first pixel; a record that is not its component's root adds its
//       sums to the root's record (u64 integer atomics, atomicMin / atomicMax for the box): one set per tile-local component.
//   k_blobs_flatten     only where label planes are asked for: label = root + 1 for a mask pixel, 0 elsewhere.
//   k_blobs_classify    every root record adds its component to the class table (LDS u64, then u64 global atomics per workgroup)
//       and competes for the largest with a u64 atomicMax of (n << 32) | (2^32 - 1 - first): of equal sizes the smaller first wins.
//   k_blobs_largest     the one record whose key won writes the query's BlobBest.
// Integer sums, minima and maxima commute: byte-identical from call to call. No float beyond out_u8 of side a.
// EVERY data-dependent loop carries the cap q.cap > the region's pixel count; a loop that reaches it (or a link that does not descend,
// or a slot outside the records) sets a bit of the error word and ends. The host turns a non-zero word into a refusal.
#include "study_device.h"

namespace musica {

constexpr uint32_t kBlobNone = 0xFFFFFFFFu;
constexpr int kBlobRuns = kSimTile / 2;          // runs of a tile row
constexpr int kBlobIds = kSimTile * kBlobRuns;   // run ids of a tile
constexpr int kBlobTrips = kSimTile / kStudyWaves;
static_assert(kSimTile == 64 && kBlobRuns == 32 && kBlobIds == 2048 && kBlobTrips == 16, "a tile row is one 64-bit word, a lane a column");
static_assert(4 * (kSimTile - 1) <= kBlobTileSlots, "a tile-local component that touches a side holds a border pixel of its own");
static_assert(kBlobClasses == 32 && kBlobWords == 6, "components, pixels, sum |d|, sum d^2, box area, border; n < 2^32");

constexpr uint32_t kBlobErrFind = 1u, kBlobErrUnion = 2u, kBlobErrLink = 4u, kBlobErrSlot = 8u;

struct BlobLoadLds {
    __device__ __forceinline__ uint32_t operator()(const uint32_t* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
struct BlobLoadGlobal {
    __device__ __forceinline__ uint32_t operator()(const uint32_t* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// The root of x: at most cap steps, every one to a smaller index (a stale word read is an older, larger ancestor: still one of the set).
template <typename Load>
__device__ __forceinline__ uint32_t blob_find(const uint32_t* par, uint32_t x, uint32_t cap, uint32_t* err, Load load) {
    for (uint32_t it = 0; it <= cap; it++) {
        const uint32_t p = load(par + x);
        if (p == x) return x;
        if (p > x) {   // never written by these kernels: end here, not outside the plane
            atomicOr(err, kBlobErrLink);
            return x;
        }
        x = p;
    }
    atomicOr(err, kBlobErrFind);
    return x;
}

// Unites the sets of a and b: the larger root goes under the smaller. Where the larger one stopped being a root between the find and
// the atomicMin, its word now holds min(what it held, b), and the union goes on from what it held: nothing that was linked is lost.
template <typename Load>
__device__ __forceinline__ void blob_union(uint32_t* par, uint32_t a, uint32_t b, uint32_t cap, uint32_t* err, Load load) {
    for (uint32_t it = 0; it <= cap; it++) {
        a = blob_find(par, a, cap, err, load);
        b = blob_find(par, b, cap, err, load);
        if (a == b) return;
        if (a < b) {
            const uint32_t s = a;
            a = b;
            b = s;
        }
        const uint32_t old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;
    }
    atomicOr(err, kBlobErrUnion);
}

__device__ __forceinline__ unsigned long long blob_starts(unsigned long long m) { return m & ~(m << 1); }
// The first column of the run of row word m that holds column x (bit x of m is set)
__device__ __forceinline__ int blob_run_start(unsigned long long m, int x) {
    const unsigned long long below = ~m & ((1ull << x) - 1ull);
    return below ? 64 - __clzll((long long)below) : 0;
}
// The id of that run in tile row `row`
__device__ __forceinline__ uint32_t blob_run_id(unsigned long long m, int row, int x) {
    return (uint32_t)(row * kBlobRuns + __popcll(blob_starts(m) & ((2ull << x) - 1ull)) - 1);
}

// A component into a class table in LDS
__device__ __forceinline__ void blob_classify(unsigned long long* cls, uint32_t n, unsigned long long sd, unsigned long long sdd, uint32_t x0, uint32_t y0, uint32_t x1,
                                              uint32_t y1, int w, int h) {
    unsigned long long* row = cls + (31 - __clz((int)n)) * kBlobWords;
    atomicAdd(row + 0, 1ull);
    atomicAdd(row + 1, (unsigned long long)n);
    atomicAdd(row + 2, sd);
    atomicAdd(row + 3, sdd);
    atomicAdd(row + 4, (unsigned long long)(x1 - x0 + 1) * (y1 - y0 + 1));
    if (x0 == 0u || y0 == 0u || x1 == (uint32_t)(w - 1) || y1 == (uint32_t)(h - 1)) atomicAdd(row + 5, 1ull);
}
__device__ __forceinline__ unsigned long long blob_key(uint32_t n, uint32_t first) { return ((unsigned long long)n << 32) | (unsigned long long)(0xFFFFFFFFu - first); }

template <int CONN>
__global__ __launch_bounds__(kStudyThreads) void k_blobs_tile(const BlobQueryDev* __restrict__ qs, uint32_t threshold, BlobScratch s, unsigned long long* __restrict__ tables) {
    __shared__ uint32_t par[kBlobIds];
    __shared__ uint32_t st_n[kBlobIds], st_sd[kBlobIds], st_sdd[kBlobIds], st_x0[kBlobIds], st_x1[kBlobIds], st_y1[kBlobIds];
    __shared__ uint8_t run_x[kBlobIds];
    __shared__ unsigned long long rowmask[kSimTile];
    __shared__ unsigned long long cls[kBlobClasses * kBlobWords];
    __shared__ unsigned long long tile_best;
    __shared__ uint32_t touching;
    const BlobQueryDev q = qs[blockIdx.z];
    const int tile = blockIdx.x;
    if (tile >= q.tiles_x * q.tiles_y) return;   // whole workgroup: the grid is sized for the query with the most tiles
    const TileGeom g = tile_geom(tile, q.tiles_x, q.w, q.h);
    const int t = threadIdx.x, l = t & 63, wave = t >> 6;
    const BlobLoadLds load;
    for (int i = t; i < kBlobClasses * kBlobWords; i += kStudyThreads) cls[i] = 0ull;
    if (t == 0) {
        tile_best = 0ull;
        touching = 0u;
    }

    // the pixels, the row masks
    uint32_t dv[kBlobTrips];
#pragma unroll
    for (int k = 0; k < kBlobTrips; k++) {
        const int r = wave + kStudyWaves * k;
        int d = 0;
        if (r < g.th && l < g.tw) {
            const int a = (int)out_u8(((const GlobalF32*)q.a)[(ptrdiff_t)(g.y0 + r) * q.a_pitch + g.x0 + l]);
            const int b = (int)((const GlobalU8*)q.b)[(ptrdiff_t)(g.y0 + r) * q.b_pitch + g.x0 + l];
            d = a > b ? a - b : b - a;
        }
        const bool on = (uint32_t)d > threshold;
        const unsigned long long m = __ballot(on);
        if (l == 0) rowmask[r] = m;
        dv[k] = on ? (uint32_t)d : 0u;
    }
    __syncthreads();

    // a run's first lane: the run as a set of its own, an empty record
#pragma unroll
    for (int k = 0; k < kBlobTrips; k++) {
        const int r = wave + kStudyWaves * k;
        const unsigned long long m = rowmask[r];
        if ((blob_starts(m) >> l) & 1ull) {
            const uint32_t id = blob_run_id(m, r, l);
            par[id] = id;
            run_x[id] = (uint8_t)l;
            st_n[id] = 0u;
            st_sd[id] = 0u;
            st_sdd[id] = 0u;
            st_x0[id] = (uint32_t)kSimTile;
            st_x1[id] = 0u;
            st_y1[id] = 0u;
        }
    }
    __syncthreads();

    // the links to the row above
#pragma unroll 1
    for (int k = 0; k < kBlobTrips; k++) {
        const int r = wave + kStudyWaves * k;
        if (r == 0) continue;
        const unsigned long long m = rowmask[r], up = rowmask[r - 1];
        if (!((m >> l) & 1ull)) continue;
        const uint32_t id = blob_run_id(m, r, l);
        if ((up >> l) & 1ull) {
            if (l == blob_run_start(m, l) || l == blob_run_start(up, l)) blob_union(par, id, blob_run_id(up, r - 1, l), q.cap, s.err, load);
        } else if (CONN == 8) {
            if (l > 0 && ((up >> (l - 1)) & 1ull)) blob_union(par, id, blob_run_id(up, r - 1, l - 1), q.cap, s.err, load);
            if (l < 63 && ((up >> (l + 1)) & 1ull)) blob_union(par, id, blob_run_id(up, r - 1, l + 1), q.cap, s.err, load);
        }
    }
    __syncthreads();

    // the runs into their roots' records, the pixels' words of the plane
    uint32_t* plane = s.parent + q.plane;
#pragma unroll
    for (int k = 0; k < kBlobTrips; k++) {
        const int r = wave + kStudyWaves * k;
        const unsigned long long m = rowmask[r];
        uint32_t s1 = dv[k], s2 = dv[k] * dv[k];
        wave_isum(s1, s2);   // all 64 lanes: the inclusive prefix along the row
        const bool on = (m >> l) & 1ull;
        const int xs = on ? blob_run_start(m, l) : 0;
        uint32_t p1 = (uint32_t)__shfl((int)s1, xs > 0 ? xs - 1 : 0, 64), p2 = (uint32_t)__shfl((int)s2, xs > 0 ? xs - 1 : 0, 64);
        if (xs == 0) p1 = p2 = 0u;
        if (r < g.th && l < g.tw) {
            const size_t at = (size_t)(g.y0 + r) * q.w + g.x0 + l;
            if (on) {
                const uint32_t root = blob_find(par, blob_run_id(m, r, l), q.cap, s.err, load);
                plane[at] = (uint32_t)((g.y0 + (int)(root >> 5)) * q.w + g.x0 + (int)run_x[root]);
                if (l == 63 || !((m >> (l + 1)) & 1ull)) {   // the run's last lane
                    atomicAdd(&st_n[root], (uint32_t)(l - xs + 1));
                    atomicAdd(&st_sd[root], s1 - p1);
                    atomicAdd(&st_sdd[root], s2 - p2);
                    atomicMin(&st_x0[root], (uint32_t)xs);
                    atomicMax(&st_x1[root], (uint32_t)l);
                    atomicMax(&st_y1[root], (uint32_t)r);
                }
            } else {
                plane[at] = kBlobNone;
            }
        }
    }
    __syncthreads();

    // the tile-local roots
    const size_t block = (q.tile0 + (size_t)tile) * kBlobTileRecords;
    BlobRecord mine = {};
    unsigned long long my_key = 0ull;
    for (int id = t; id < kBlobIds; id += kStudyThreads) {
        const int row = id >> 5;
        if ((id & 31) >= __popcll(blob_starts(rowmask[row])) || par[id] != (uint32_t)id) continue;
        BlobRecord rec;
        rec.first = rec.root = (uint32_t)((g.y0 + row) * q.w + g.x0 + (int)run_x[id]);
        rec.n = st_n[id];
        rec.x0 = (uint32_t)g.x0 + st_x0[id];
        rec.y0 = (uint32_t)(g.y0 + row);
        rec.x1 = (uint32_t)g.x0 + st_x1[id];
        rec.y1 = (uint32_t)g.y0 + st_y1[id];
        rec.pad = 0u;
        rec.sd = st_sd[id];
        rec.sdd = st_sdd[id];
        if (st_x0[id] == 0u || st_x1[id] == (uint32_t)(g.tw - 1) || row == 0 || st_y1[id] == (uint32_t)(g.th - 1)) {
            const uint32_t slot = atomicAdd(&touching, 1u);
            if (slot < (uint32_t)kBlobTileSlots) {
                s.recs[block + slot] = rec;
                s.slots[q.plane + rec.first] = (uint32_t)(block + slot);
            } else {
                atomicOr(s.err, kBlobErrSlot);
            }
        } else {
            blob_classify(cls, rec.n, rec.sd, rec.sdd, rec.x0, rec.y0, rec.x1, rec.y1, q.w, q.h);
            const unsigned long long key = blob_key(rec.n, rec.first);
            if (key > my_key) {
                my_key = key;
                mine = rec;
            }
        }
    }
    if (my_key) atomicMax(&tile_best, my_key);
    __syncthreads();
    for (int i = t; i < kBlobClasses * kBlobWords; i += kStudyThreads)
        if (cls[i]) atomicAdd((unsigned long long*)((GlobalU64*)tables + q.table + i), cls[i]);
    const unsigned long long best = tile_best;
    if (best ? my_key == best : t == 0) s.recs[block + kBlobTileSlots] = mine;   // the tile's largest inner component; n = 0: none
    if (t == 0) {
        s.counts[q.tile0 + tile] = touching < (uint32_t)kBlobTileSlots ? touching : (uint32_t)kBlobTileSlots;
        if (best) atomicMax(s.best + blockIdx.z, best);
    }
}

// kBlobSeamThreads threads a tile: thread j < 64 row j of its last column, thread 64 + i column i of its last row
template <int CONN>
__global__ __launch_bounds__(kBlobSeamThreads) void k_blobs_seam(const BlobQueryDev* __restrict__ qs, BlobScratch s) {
    const BlobQueryDev q = qs[blockIdx.z];
    const int tile = blockIdx.x;
    if (tile >= q.tiles_x * q.tiles_y) return;
    const TileGeom g = tile_geom(tile, q.tiles_x, q.w, q.h);
    uint32_t* plane = s.parent + q.plane;
    const BlobLoadGlobal load;
    const auto at = [&](int x, int y) { return (uint32_t)(y * q.w + x); };
    const auto on = [&](int x, int y) { return x >= 0 && y >= 0 && x < q.w && y < q.h && plane[at(x, y)] != kBlobNone; };
    const auto join = [&](int x0, int y0, int x1, int y1) { blob_union(plane, at(x0, y0), at(x1, y1), q.cap, s.err, load); };
    const int j = threadIdx.x;
    if (j < kSimTile) {
        const int x = g.x0 + kSimTile - 1, y = g.y0 + j;
        if (g.tw < kSimTile || x + 1 >= q.w || j >= g.th || !on(x, y)) return;
        // (x, y) - (x + 1, y): not where the pair above, inside the same two tiles, unites the same two tile-local components
        if (on(x + 1, y) && !(j > 0 && on(x, y - 1) && on(x + 1, y - 1))) join(x, y, x + 1, y);
        if (CONN == 8) {   // a diagonal is needed only where neither straight pair beside it exists
            if (on(x + 1, y + 1) && !on(x + 1, y) && !on(x, y + 1)) join(x, y, x + 1, y + 1);
            if (on(x + 1, y - 1) && !on(x + 1, y) && !on(x, y - 1)) join(x, y, x + 1, y - 1);
        }
    } else {
        const int i = j - kSimTile, x = g.x0 + i, y = g.y0 + kSimTile - 1;
        if (g.th < kSimTile || y + 1 >= q.h || i >= g.tw || !on(x, y)) return;
        if (on(x, y + 1) && !(i > 0 && on(x - 1, y) && on(x - 1, y + 1))) join(x, y, x, y + 1);
        if (CONN == 8) {
            if (on(x + 1, y + 1) && !on(x, y + 1) && !on(x + 1, y)) join(x, y, x + 1, y + 1);
            if (on(x - 1, y + 1) && !on(x, y + 1) && !on(x - 1, y)) join(x, y, x - 1, y + 1);
        }
    }
}

__global__ __launch_bounds__(kStudyThreads) void k_blobs_flush(const BlobQueryDev* __restrict__ qs, BlobScratch s, unsigned long long records) {
    const BlobQueryDev q = qs[blockIdx.z];
    const int tile = blockIdx.x;
    if (tile >= q.tiles_x * q.tiles_y || threadIdx.x >= s.counts[q.tile0 + tile]) return;
    BlobRecord* rec = s.recs + (q.tile0 + (size_t)tile) * kBlobTileRecords + threadIdx.x;
    uint32_t* plane = s.parent + q.plane;
    const uint32_t first = rec->first;
    const uint32_t root = blob_find(plane, first, q.cap, s.err, BlobLoadGlobal());
    if (root == first) return;
    const uint32_t slot = s.slots[q.plane + root];   // a root under which another tile's component hangs touches a side of its own tile
    if (slot >= records) {
        atomicOr(s.err, kBlobErrSlot);
        return;
    }
    rec->root = root;
    plane[first] = root;   // a shorter walk for k_blobs_flatten; still an ancestor, still smaller
    BlobRecord* to = s.recs + slot;
    atomicAdd(&to->n, rec->n);
    atomicAdd(&to->sd, rec->sd);
    atomicAdd(&to->sdd, rec->sdd);
    atomicMin(&to->x0, rec->x0);
    atomicMin(&to->y0, rec->y0);
    atomicMax(&to->x1, rec->x1);
    atomicMax(&to->y1, rec->y1);
}

__global__ __launch_bounds__(kStudyThreads) void k_blobs_flatten(const BlobQueryDev* __restrict__ qs, BlobScratch s) {
    const BlobQueryDev q = qs[blockIdx.z];
    const size_t i = (size_t)blockIdx.x * kStudyThreads + threadIdx.x;
    if (i >= (size_t)q.w * q.h) return;
    const uint32_t* plane = s.parent + q.plane;
    s.labels[q.plane + i] = plane[i] == kBlobNone ? 0u : blob_find(plane, (uint32_t)i, q.cap, s.err, BlobLoadGlobal()) + 1u;
}

__global__ __launch_bounds__(kStudyThreads) void k_blobs_classify(const BlobQueryDev* __restrict__ qs, BlobScratch s, unsigned long long* __restrict__ tables) {
    __shared__ unsigned long long cls[kBlobClasses * kBlobWords];
    __shared__ unsigned long long group_best;
    const BlobQueryDev q = qs[blockIdx.z];
    const int tile = blockIdx.x, t = threadIdx.x;
    if (tile >= q.tiles_x * q.tiles_y) return;
    const uint32_t count = s.counts[q.tile0 + tile];
    if (count == 0u) return;   // whole workgroup
    for (int i = t; i < kBlobClasses * kBlobWords; i += kStudyThreads) cls[i] = 0ull;
    if (t == 0) group_best = 0ull;
    __syncthreads();
    if ((uint32_t)t < count) {
        const BlobRecord rec = s.recs[(q.tile0 + (size_t)tile) * kBlobTileRecords + t];
        if (rec.root == rec.first) {
            blob_classify(cls, rec.n, rec.sd, rec.sdd, rec.x0, rec.y0, rec.x1, rec.y1, q.w, q.h);
            atomicMax(&group_best, blob_key(rec.n, rec.first));
        }
    }
    __syncthreads();
    for (int i = t; i < kBlobClasses * kBlobWords; i += kStudyThreads)
        if (cls[i]) atomicAdd((unsigned long long*)((GlobalU64*)tables + q.table + i), cls[i]);
    if (t == 0 && group_best) atomicMax(s.best + blockIdx.z, group_best);
}

__global__ __launch_bounds__(kStudyThreads) void k_blobs_largest(const BlobQueryDev* __restrict__ qs, BlobScratch s) {
    const BlobQueryDev q = qs[blockIdx.z];
    const int tile = blockIdx.x, t = threadIdx.x;
    if (tile >= q.tiles_x * q.tiles_y) return;
    const unsigned long long best = s.best[blockIdx.z];
    if (best == 0ull) return;   // nothing changed: the zeroed BlobBest stands
    const uint32_t count = s.counts[q.tile0 + tile];
    const BlobRecord* block = s.recs + (q.tile0 + (size_t)tile) * kBlobTileRecords;
    for (int k = t; k <= kBlobTileSlots; k += kStudyThreads) {
        if (k < kBlobTileSlots && (uint32_t)k >= count) continue;
        const BlobRecord rec = block[k];
        if (rec.n == 0u || rec.root != rec.first || blob_key(rec.n, rec.first) != best) continue;
        BlobBest b;
        b.n = rec.n;
        b.first = rec.first;
        b.x0 = rec.x0;
        b.y0 = rec.y0;
        b.x1 = rec.x1;
        b.y1 = rec.y1;
        b.sdd = rec.sdd;
        s.largest[blockIdx.z] = b;
    }
}

void launch_sim_blobs(hipStream_t st, const BlobQueryDev* d_qs, int count, int max_tiles, unsigned long long max_pixels, unsigned long long records, uint32_t threshold,
                      int connectivity, const BlobScratch& s, unsigned long long* tables) {
    const dim3 grid((unsigned)max_tiles, 1, (unsigned)count), block(kStudyThreads);
    if (connectivity == 8) {
        hipLaunchKernelGGL(k_blobs_tile<8>, grid, block, 0, st, d_qs, threshold, s, tables);
        hipLaunchKernelGGL(k_blobs_seam<8>, grid, dim3(kBlobSeamThreads), 0, st, d_qs, s);
    } else {
        hipLaunchKernelGGL(k_blobs_tile<4>, grid, block, 0, st, d_qs, threshold, s, tables);
        hipLaunchKernelGGL(k_blobs_seam<4>, grid, dim3(kBlobSeamThreads), 0, st, d_qs, s);
    }
    hipLaunchKernelGGL(k_blobs_flush, grid, block, 0, st, d_qs, s, records);
    if (s.labels)
        hipLaunchKernelGGL(k_blobs_flatten, dim3((unsigned)((max_pixels + kStudyThreads - 1) / kStudyThreads), 1, (unsigned)count), block, 0, st, d_qs, s);
    hipLaunchKernelGGL(k_blobs_classify, grid, block, 0, st, d_qs, s, tables);
    hipLaunchKernelGGL(k_blobs_largest, grid, block, 0, st, d_qs, s);
}

}  // namespace musica
