// musica_study.hip — the metamorphic study's entry points of include/musica.h: the reference slots and the query calls (musica_sim_*),
// the ensemble accumulators (musica_sim_ensemble_*) and the alterations of the input (musica_alter_*). Their kernels: kernels_similarity.hip,
// kernels_joint.hip, kernels_displace.hip, kernels_scales.hip, kernels_ensemble.hip, kernels_covariance.hip, kernels_alteration.hip,
// kernels_symmetry.hip, kernels_blur.hip, kernels_codec.hip, kernels_zoom.hip, kernels_scatter.hip, kernels_warp.hip and, each with a measurement and an alteration,
// kernels_details.hip, kernels_edges.hip, kernels_gratings.hip, kernels_points.hip, kernels_gain.hip, kernels_levels.hip, kernels_gradients.hip, kernels_order.hip, kernels_lattice.hip, kernels_blobs.hip, kernels_spectrum.hip, kernels_cooccurrence.hip, kernels_granulometry.hip, kernels_contours.hip, kernels_minkowski.hip and kernels_reach.hip, and the measurement of kernels_observer.hip. Their state is musica_ctx::study; the pipeline
// (musica_ctx.hip, musica_step.hip) knows none of it. Calls of one kind share a host frame: sim_derive_slot (a slot made from a slot),
// sim_patch_list (the list measurements), sim_query_tables (the table comparisons) and alter_into (the alterations with an entry point).
#include <math.h>
#include <string.h>

#include "musica_ctx.h"

// ---- helpers (templates among them, so they stand outside the extern "C" block) -------------------------------------------------------
// A device buffer sized for one call of `fn` (or a `twin` pair that grows together), regrown when a call needs more than the largest
// call so far: *cap and `want` count units of `per` elements; a refusal names `want` in `unit`s (nullptr: in bytes).
template <typename T, typename U = T>
static int grow(musica_ctx* c, const char* fn, T** buf, size_t* cap, size_t want, const char* unit = nullptr, size_t per = 1, U** twin = nullptr) {
    if (want <= *cap) return 1;
    HIP_OK(drelease(c, buf));
    if (twin) HIP_OK(drelease(c, twin));
    *cap = 0;
    if (!dalloc(c, buf, per * want) || (twin && !dalloc(c, twin, per * want)))
        return unit ? fail("%s: device allocation of %zu %s failed", fn, want, unit) : fail("%s: device allocation of %zu bytes failed", fn, want * sizeof(T));
    *cap = want;
    return 1;
}

// The grid of MUSICA_SIM_TILE^2 tiles of the regions of one launch: each region's tiles_x x tiles_y, where its tiles' tables start in
// the launch's tile-table buffer (`per_tile` elements per tile, region after region) and the largest grid (the launch's grid.x).
static int tiles_along(uint32_t len) { return (int)((len + MUSICA_SIM_TILE - 1) / MUSICA_SIM_TILE); }
struct TileRun {
    size_t next = 0;      // elements so far: the next region's tile_base
    int max_tiles = 1;
    template <typename D>
    void place(D& d, size_t per_tile) {
        d.tiles_x = tiles_along((uint32_t)d.w);
        d.tiles_y = tiles_along((uint32_t)d.h);
        d.tile_base = next;
        next += (size_t)d.tiles_x * d.tiles_y * per_tile;
        max_tiles = std::max(max_tiles, d.tiles_x * d.tiles_y);
    }
};

static size_t sim_side(const musica_ctx* c) { return (size_t)c->N - 2 * MUSICA_OUT_MARGIN; }   // of a slot's plane: the cropped output

// The plane of a slot that `fn` is about to write, allocated on first use, after the two refusals every writer shares.
static uint8_t* sim_slot_for_write(musica_ctx* c, const char* fn, uint32_t slot) {
    if (c->N <= 2 * MUSICA_OUT_MARGIN) { fail("%s: image too small for the %d-pixel margin", fn, MUSICA_OUT_MARGIN); return nullptr; }
    if (hipSetDevice(c->p.device) != hipSuccess) { fail("%s: hipSetDevice failed", fn); return nullptr; }
    if (!ensure(c, &c->study.slot[slot], sim_side(c) * sim_side(c))) { fail("musica_sim: device allocation of slot %u failed", slot); return nullptr; }
    return c->study.slot[slot];
}

// The calls that make dst_slot from src_slot, behind their NULL refusals: what they refuse about the pair, then `check` (the call's
// refusals about its other arguments: 1, or fail(...)), then launch(src, dst) into the destination's plane. A written source implies a
// context larger than the margin (only sim_slot_for_write's callers set `written`), so its margin refusal cannot fire behind the pair's.
template <typename Check, typename Launch>
static int sim_derive_slot(musica_ctx* c, const char* fn, uint32_t dst_slot, uint32_t src_slot, Check check, Launch launch) {
    if (dst_slot >= MUSICA_SIM_SLOTS || src_slot >= MUSICA_SIM_SLOTS) return fail("%s: slot %u / %u >= %d", fn, dst_slot, src_slot, MUSICA_SIM_SLOTS);
    if (dst_slot == src_slot) return fail("%s: dst_slot == src_slot (%u)", fn, dst_slot);
    if (!c->study.written[src_slot]) return fail("%s: slot %u was never written", fn, src_slot);
    if (!check()) return 0;
    uint8_t* dst = sim_slot_for_write(c, fn, dst_slot);
    if (!dst) return 0;
    launch(c->study.slot[src_slot], dst);
    HIP_OK(hipGetLastError());
    c->study.written[dst_slot] = true;
    return 1;
}

static uint32_t gcd_u32(uint32_t a, uint32_t b) { return b ? gcd_u32(b, a % b) : a; }

static_assert(kZoomMaxP == MUSICA_ZOOM_MAX_P, "kernels_zoom.hip's u32 sums hold for the zooms of include/musica.h");

// What both zoom calls refuse about p / q: harness.zoom's 1 <= q < p <= MUSICA_ZOOM_MAX_P in lowest terms.
static int zoom_check(const char* fn, uint32_t p, uint32_t q) {
    if (q == 0 || p <= q || p > MUSICA_ZOOM_MAX_P) return fail("%s: zoom %u / %u is not 1 <= q < p <= %d", fn, p, q, MUSICA_ZOOM_MAX_P);
    if (gcd_u32(p, q) != 1) return fail("%s: zoom %u / %u is not in lowest terms (gcd %u)", fn, p, q, gcd_u32(p, q));
    return 1;
}

// What both codec calls refuse about a table that is not NULL and an origin, as processing.codec_table_words does; then the table as the
// kernel takes it. No device work.
static int codec_check(const char* fn, const uint16_t* table, uint32_t origin, CodecTable& t) {
    if (origin > 7) return fail("%s: origin %u is not in 0 .. 7", fn, origin);
    for (int k = 0; k < 64; k++) {
        if (table[k] == 0) return fail("%s: table entry %d (v = %d, u = %d) is 0: the steps are 1 .. 65535", fn, k, k / 8, k % 8);
        t.q[k] = table[k];
    }
    return 1;
}
static_assert(kScatterMaxRadius == MUSICA_SCATTER_MAX_RADIUS && kScatterMaxDen == MUSICA_SCATTER_MAX_DEN,
              "kernels_scatter.hip's u32 row plane and u64 numerator hold for the scatters of include/musica.h");

// What both scatter calls refuse about (radius, num / den): harness.scatter's 1 <= radius <= MUSICA_SCATTER_MAX_RADIUS and
// 1 <= num < den <= MUSICA_SCATTER_MAX_DEN in lowest terms.
static int scatter_check(const char* fn, uint32_t radius, uint32_t num, uint32_t den) {
    if (radius < 1 || radius > MUSICA_SCATTER_MAX_RADIUS) return fail("%s: radius %u out of range [1, %d]", fn, radius, MUSICA_SCATTER_MAX_RADIUS);
    if (num == 0 || num >= den || den > MUSICA_SCATTER_MAX_DEN)
        return fail("%s: scatter fraction %u / %u is not 1 <= num < den <= %d", fn, num, den, MUSICA_SCATTER_MAX_DEN);
    if (gcd_u32(den, num) != 1) return fail("%s: scatter fraction %u / %u is not in lowest terms (gcd %u)", fn, num, den, gcd_u32(den, num));
    return 1;
}

static_assert(kWarpGrid == MUSICA_WARP_GRID && kWarpUnit == MUSICA_WARP_UNIT && kWarpMaxShift == MUSICA_WARP_MAX_SHIFT,
              "kernels_warp.hip's cells, window and i32 sums hold for the fields of include/musica.h");
static_assert(MUSICA_WARP_MAX_NODES == ((16384 - 2 * MUSICA_OUT_MARGIN - 1 + MUSICA_WARP_GRID - 1) >> 6) + 2, "the nodes of the largest plane at the largest origin");

// What both warp calls refuse about a field of nodes x nodes nodes for a plane of side n at `origin`, as processing.warp_field does; then
// the m x m nodes the plane needs, packed for the device (dx in the low half of a u32, dy in the high one). No device work.
static int warp_check(const char* fn, const int16_t* field, uint32_t nodes, uint32_t origin, size_t n, std::vector<uint32_t>& packed, int* m) {
    if (origin >= MUSICA_WARP_GRID) return fail("%s: origin %u is not in 0 .. %d", fn, origin, MUSICA_WARP_GRID - 1);
    const uint32_t need = (uint32_t)((n - 1 + origin) >> 6) + 2;
    if (nodes < need) return fail("%s: %u nodes a side are fewer than the %u that a plane of %zu pixels at origin %u needs", fn, nodes, need, n, origin);
    if (nodes > MUSICA_WARP_MAX_NODES) return fail("%s: %u nodes a side are more than %d", fn, nodes, MUSICA_WARP_MAX_NODES);
    for (uint32_t j = 0; j < nodes; j++)
        for (uint32_t i = 0; i < nodes; i++)
            for (int k = 0; k < 2; k++) {
                const int v = field[((size_t)j * nodes + i) * 2 + k];
                if (v < -MUSICA_WARP_MAX_SHIFT || v > MUSICA_WARP_MAX_SHIFT)
                    return fail("%s: node (row %u, column %u) has the component %d, beyond +-%d", fn, j, i, v, MUSICA_WARP_MAX_SHIFT);
            }
    packed.resize((size_t)need * need);
    for (uint32_t j = 0; j < need; j++)
        for (uint32_t i = 0; i < need; i++) {
            const int16_t* d = field + ((size_t)j * nodes + i) * 2;
            packed[(size_t)j * need + i] = (uint32_t)(uint16_t)d[0] | (uint32_t)(uint16_t)d[1] << 16;
        }
    *m = (int)need;
    return 1;
}

// The call's nodes on the device, in the context's buffer (grown when a call needs more than the largest so far): copied on the
// stream, behind the kernel that still reads the last call's, and `packed` is free again when this returns.
static int warp_upload(musica_ctx* c, const char* fn, const std::vector<uint32_t>& packed) {
    if (!grow(c, fn, &c->study.d_warp_nodes, &c->study.warp_nodes_cap, packed.size(), "nodes")) return 0;
    HIP_OK(hipMemcpyAsync(c->study.d_warp_nodes, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 1;
}

// The u32 plane between the two scatter launches, allocated on first use and freed with the context.
static int scatter_plane(musica_ctx* c, const char* fn) {
    const size_t nn = (size_t)c->N * c->N;
    if (!ensure(c, &c->study.d_scatter, nn)) return fail("%s: device allocation of the %zu-byte row plane failed", fn, nn * sizeof(uint32_t));
    return 1;
}

// ---- lists of square patches on a plane (the details' boxes, the edges' and gratings' plates) -----------------------------------------
// What a refusal calls a relation's patch and its item: "box" / "boxes" of a "detail", "plate" / "plates" of an "edge" or a "grating".
struct PatchNouns {
    const char *square, *squares, *item;
};
constexpr PatchNouns kDetailNouns{"box", "boxes", "detail"}, kEdgeNouns{"plate", "plates", "edge"}, kGratingNouns{"plate", "plates", "grating"},
    kPointNouns{"window", "windows", "point"};

// What every list call refuses about `count` items (each with a centre x, y) for a plane of side n, as processing's *_list do: the
// count; per item what each(i, item, packed) refuses about it (1, or fail(...); it fills the packed item for the device) and a square
// centre +- reach(item) that leaves the plane; squares that are not pairwise disjoint. No device work.
template <typename Item, typename Packed, typename Reach, typename Each>
static int patch_list_check(const char* fn, const PatchNouns& nouns, uint32_t count, uint32_t most, const Item* items, int n, std::vector<Packed>& packed,
                            Reach reach, Each each) {
    if (count == 0 || count > most) return fail("%s: count %u out of range [1, %d]", fn, count, (int)most);
    packed.resize(count);
    for (uint32_t i = 0; i < count; i++) {
        const Item& t = items[i];
        if (!each(i, t, packed[i])) return 0;
        const int64_t r = reach(t);
        if (t.x - r < 0 || t.y - r < 0 || t.x + r >= n || t.y + r >= n)
            return fail("%s: %s %u: the %s (%d, %d) +- %d leaves the %d x %d plane", fn, nouns.item, i, nouns.square, t.x, t.y, (int)r, n, n);
    }
    for (uint32_t i = 0; i < count; i++)
        for (uint32_t j = i + 1; j < count; j++) {
            const int64_t both = reach(items[i]) + reach(items[j]);
            if (std::abs((int64_t)items[i].x - items[j].x) <= both && std::abs((int64_t)items[i].y - items[j].y) <= both)
                return fail("%s: the %s of %ss %u and %u are not disjoint", fn, nouns.squares, nouns.item, i, j);
        }
    return 1;
}

static_assert(kDetailMaxRadius == MUSICA_DETAIL_MAX_RADIUS && kDetailMaxContrast == MUSICA_DETAIL_MAX_CONTRAST && kDetailMax == MUSICA_DETAIL_MAX,
              "kernels_details.hip's tile list, u32 pixel and u32 partial sums hold for the details of include/musica.h");
static_assert(sizeof(musica_sim_detail_result) == kDetailWords * sizeof(uint64_t), "k_sim_details writes a musica_sim_detail_result as its u64 words");

// What both detail calls refuse about a list for a plane of side n (processing.detail_list): patch_list_check with each radius (and
// each contrast when the call looks at it) and the boxes' reach 2r + 2.
static int details_check(const char* fn, uint32_t count, const musica_detail* ds, int n, bool with_contrast, std::vector<PackedDetail>& packed) {
    return patch_list_check(fn, kDetailNouns, count, MUSICA_DETAIL_MAX, ds, n, packed, [](const musica_detail& d) { return 2 * (int64_t)d.radius + 2; },
                            [&](uint32_t i, const musica_detail& d, PackedDetail& p) {
                                if (d.radius < 1 || d.radius > MUSICA_DETAIL_MAX_RADIUS)
                                    return fail("%s: detail %u: radius %u out of range [1, %d]", fn, i, d.radius, MUSICA_DETAIL_MAX_RADIUS);
                                if (with_contrast && (d.contrast == 0 || d.contrast < -MUSICA_DETAIL_MAX_CONTRAST || d.contrast > MUSICA_DETAIL_MAX_CONTRAST))
                                    return fail("%s: detail %u: contrast %d is not 1 <= |contrast| <= %d", fn, i, d.contrast, MUSICA_DETAIL_MAX_CONTRAST);
                                const int c = with_contrast ? d.contrast : 0;
                                p = {(uint32_t)d.x | ((uint32_t)d.y << 16), d.radius | ((uint32_t)(c + 512) << 8)};
                                return 1;
                            });
}

static_assert(kEdgeMinHalf == MUSICA_EDGE_MIN_HALF && kEdgeMaxHalf == MUSICA_EDGE_MAX_HALF && kEdgeMinQ == MUSICA_EDGE_MIN_Q && kEdgeMaxQ == MUSICA_EDGE_MAX_Q &&
                  kEdgeMaxContrast == MUSICA_EDGE_MAX_CONTRAST && kEdgeMax == MUSICA_EDGE_MAX && kEdgeBinsMax == MUSICA_EDGE_BINS_MAX,
              "kernels_edges.hip's tile list, u32 pixel, LDS table and u32 sums hold for the edges of include/musica.h");
static_assert(sizeof(musica_sim_edge_result) == kEdgeWords * sizeof(uint64_t), "k_sim_edges writes a musica_sim_edge_result as its u64 words");

uint32_t musica_edge_bins(uint32_t half, uint32_t p, uint32_t q) {
    if (half < MUSICA_EDGE_MIN_HALF || half > MUSICA_EDGE_MAX_HALF || q < MUSICA_EDGE_MIN_Q || q > MUSICA_EDGE_MAX_Q || p < 1 || p >= q || gcd_u32(p, q) != 1) return 0;
    return 2 * ((4 * (q + p) * half + q - 1) / q) + 1;
}

// What both edge calls refuse about a list for a plane of side n (processing.edge_list): patch_list_check with each half-side, slope
// and orientation (and each contrast when the call looks at it) and the plates' reach 2 half. Each edge's table lies behind the one
// before it; `words` is the tables' total.
static int edges_check(const char* fn, uint32_t count, const musica_edge* es, int n, bool with_contrast, std::vector<PackedEdge>& packed, uint64_t* words) {
    *words = 0;
    return patch_list_check(fn, kEdgeNouns, count, MUSICA_EDGE_MAX, es, n, packed, [](const musica_edge& e) { return 2 * (int64_t)e.half; },
                            [&](uint32_t i, const musica_edge& e, PackedEdge& p) {
                                if (e.half < MUSICA_EDGE_MIN_HALF || e.half > MUSICA_EDGE_MAX_HALF)
                                    return fail("%s: edge %u: half-side %u out of range [%d, %d]", fn, i, e.half, MUSICA_EDGE_MIN_HALF, MUSICA_EDGE_MAX_HALF);
                                const uint32_t bins = musica_edge_bins(e.half, e.p, e.q);
                                if (!bins)
                                    return fail("%s: edge %u: slope %u / %u is not 1 <= p < q, %d <= q <= %d in lowest terms", fn, i, e.p, e.q, MUSICA_EDGE_MIN_Q, MUSICA_EDGE_MAX_Q);
                                if (e.orientation > 3) return fail("%s: edge %u: orientation %u out of range [0, 3]", fn, i, e.orientation);
                                if (with_contrast && (e.contrast == 0 || e.contrast < -MUSICA_EDGE_MAX_CONTRAST || e.contrast > MUSICA_EDGE_MAX_CONTRAST))
                                    return fail("%s: edge %u: contrast %d is not 1 <= |contrast| <= %d", fn, i, e.contrast, MUSICA_EDGE_MAX_CONTRAST);
                                p = {(uint32_t)e.x | ((uint32_t)e.y << 16), e.half | (e.p << 8) | (e.q << 16) | (e.orientation << 24), with_contrast ? e.contrast : 0,
                                     (uint32_t)*words};
                                *words += 4ull * bins;
                                return 1;
                            });
}

static_assert(kGratingMinHalf == MUSICA_GRATING_MIN_HALF && kGratingMaxHalf == MUSICA_GRATING_MAX_HALF && kGratingMaxU == MUSICA_GRATING_MAX_U &&
                  kGratingMaxPeriod == MUSICA_GRATING_MAX_PERIOD && kGratingMaxContrast == MUSICA_GRATING_MAX_CONTRAST && kGratingMax == MUSICA_GRATING_MAX,
              "kernels_gratings.hip's tile list, u32 pixel, LDS tables and u32 sums hold for the gratings of include/musica.h");
static_assert(sizeof(musica_sim_grating_result) == kGratingWords * sizeof(uint64_t), "k_sim_gratings writes a musica_sim_grating_result as its u64 words");

// What both grating calls refuse about a list for a plane of side n (processing.grating_list): patch_list_check with each half-side,
// wave vector and period and the plates' reach 2 half. Each grating's wave (and a quarter of its table's place) lies behind the one
// before it; `periods` is the periods' sum.
static int gratings_check(const char* fn, uint32_t count, const musica_grating* gs, int n, std::vector<PackedGrating>& packed, uint64_t* periods) {
    *periods = 0;
    return patch_list_check(fn, kGratingNouns, count, MUSICA_GRATING_MAX, gs, n, packed, [](const musica_grating& g) { return 2 * (int64_t)g.half; },
                            [&](uint32_t i, const musica_grating& g, PackedGrating& p) {
                                if (g.half < MUSICA_GRATING_MIN_HALF || g.half > MUSICA_GRATING_MAX_HALF)
                                    return fail("%s: grating %u: half-side %u out of range [%d, %d]", fn, i, g.half, MUSICA_GRATING_MIN_HALF, MUSICA_GRATING_MAX_HALF);
                                if (g.ux < -MUSICA_GRATING_MAX_U || g.ux > MUSICA_GRATING_MAX_U || g.uy < -MUSICA_GRATING_MAX_U || g.uy > MUSICA_GRATING_MAX_U ||
                                    gcd_u32((uint32_t)std::abs(g.ux), (uint32_t)std::abs(g.uy)) != 1)
                                    return fail("%s: grating %u: wave vector (%d, %d) is not coprime with |ux|, |uy| <= %d", fn, i, g.ux, g.uy, MUSICA_GRATING_MAX_U);
                                if (g.period < 2 || g.period > MUSICA_GRATING_MAX_PERIOD || g.period > g.half || 2 * (uint32_t)std::abs(g.ux) > g.period ||
                                    2 * (uint32_t)std::abs(g.uy) > g.period)
                                    return fail("%s: grating %u: period %u is not 2 <= T <= min(%d, half) with 2 |ux|, 2 |uy| <= T", fn, i, g.period, MUSICA_GRATING_MAX_PERIOD);
                                p = {(uint32_t)g.x | ((uint32_t)g.y << 16), g.half | (g.period << 8) | (((uint32_t)g.ux & 0xFFu) << 16) | (((uint32_t)g.uy & 0xFFu) << 24),
                                     (uint32_t)*periods};
                                *periods += g.period;
                                return 1;
                            });
}

static_assert(kPointMinRadius == MUSICA_POINT_MIN_RADIUS && kPointMaxRadius == MUSICA_POINT_MAX_RADIUS && kPointMaxSize == MUSICA_POINT_MAX_SIZE &&
                  kPointMinContrast == MUSICA_POINT_MIN_CONTRAST && kPointMaxContrast == MUSICA_POINT_MAX_CONTRAST && kPointMaxGroups == MUSICA_POINT_MAX_GROUPS &&
                  kPointMax == MUSICA_POINT_MAX,
              "kernels_points.hip's tile list, u32 pixel and u32 sums hold for the points of include/musica.h");
static_assert(sizeof(musica_sim_point_result) == kPointWords * sizeof(uint64_t), "k_sim_points writes a musica_sim_point_result as its u64 words");

// What both point calls refuse about a list for a plane of side n (processing.point_list): `groups` itself, then patch_list_check with
// each radius (one for the whole list), size, contrast (when the call looks at it) and group, and the windows' reach R.
static int points_check(const char* fn, uint32_t count, const musica_defect* ps, int n, bool with_contrast, uint32_t groups, std::vector<PackedPoint>& packed) {
    if (groups < 1 || groups > MUSICA_POINT_MAX_GROUPS) return fail("%s: groups %u out of range [1, %d]", fn, groups, MUSICA_POINT_MAX_GROUPS);
    return patch_list_check(fn, kPointNouns, count, MUSICA_POINT_MAX, ps, n, packed, [](const musica_defect& d) { return (int64_t)d.radius; },
                            [&](uint32_t i, const musica_defect& d, PackedPoint& p) {
                                if (d.radius < MUSICA_POINT_MIN_RADIUS || d.radius > MUSICA_POINT_MAX_RADIUS)
                                    return fail("%s: point %u: radius %u out of range [%d, %d]", fn, i, d.radius, MUSICA_POINT_MIN_RADIUS, MUSICA_POINT_MAX_RADIUS);
                                if (d.radius != ps[0].radius)
                                    return fail("%s: point %u: radius %u differs from the list's radius %u", fn, i, d.radius, ps[0].radius);
                                if (d.size < 1 || d.size > MUSICA_POINT_MAX_SIZE) return fail("%s: point %u: size %u out of range [1, %d]", fn, i, d.size, MUSICA_POINT_MAX_SIZE);
                                if (with_contrast && (d.contrast == 0 || d.contrast < MUSICA_POINT_MIN_CONTRAST || d.contrast > MUSICA_POINT_MAX_CONTRAST))
                                    return fail("%s: point %u: contrast %d is not in [%d, %d] without 0", fn, i, d.contrast, MUSICA_POINT_MIN_CONTRAST,
                                                MUSICA_POINT_MAX_CONTRAST);
                                if (d.group >= groups) return fail("%s: point %u: group %u is not below %u", fn, i, d.group, groups);
                                const int c = with_contrast ? d.contrast : 0;
                                p = {(uint32_t)d.x | ((uint32_t)d.y << 16), d.radius | (d.size << 6) | (d.group << 8) | ((uint32_t)(c - MUSICA_POINT_MIN_CONTRAST) << 12)};
                                return 1;
                            });
}

// Where a relation's list calls keep their device buffers in musica_ctx::study, and how large: the list's `most` items, and for the
// measurement `out_words` u64 of results per item and `tables_cap` u32 of tables (tables == nullptr: the measurement has none).
template <typename Packed>
struct PatchBuffers {
    const char* item;
    Packed* StudyState::*list;
    size_t most;
    unsigned long long* StudyState::*out;
    size_t out_words;
    uint32_t* StudyState::*tables;
    size_t tables_cap;
};
constexpr PatchBuffers<PackedDetail> kDetailBuffers{"detail", &StudyState::d_details, MUSICA_DETAIL_MAX, &StudyState::d_detail_out, kDetailWords, nullptr, 0};
constexpr PatchBuffers<PackedEdge> kEdgeBuffers{"edge", &StudyState::d_edges, MUSICA_EDGE_MAX, &StudyState::d_edge_out, kEdgeWords, &StudyState::d_edge_tables,
                                                (size_t)MUSICA_EDGE_MAX * 4 * MUSICA_EDGE_BINS_MAX};
constexpr PatchBuffers<PackedGrating> kGratingBuffers{"grating", &StudyState::d_gratings, MUSICA_GRATING_MAX, &StudyState::d_grating_out, kGratingWords,
                                                      &StudyState::d_grating_tables, (size_t)MUSICA_GRATING_MAX * 4 * MUSICA_GRATING_MAX_PERIOD};
// the stacks' buffer also holds the launch plan of k_sim_points, behind the largest tables
// ... and the list's the tile rows' ranges of k_alter_points, behind the points
constexpr PatchBuffers<PackedPoint> kPointBuffers{"point", &StudyState::d_points, MUSICA_POINT_MAX + kPointTileRows, &StudyState::d_point_out, kPointWords, &StudyState::d_point_tables,
                                                  (size_t)kPointTableWords + kPointPlanWords};

// The call's list on the device, in the relation's buffer (allocated on first use): copied on the stream, behind the kernels that
// still read the last call's, and `packed` is free again when this returns.
template <typename Packed>
static int upload_list(musica_ctx* c, const char* fn, const PatchBuffers<Packed>& bufs, const std::vector<Packed>& packed) {
    if (!ensure(c, &(c->study.*bufs.list), bufs.most)) return fail("%s: device allocation of the %s list failed", fn, bufs.item);
    HIP_OK(hipMemcpyAsync(c->study.*bufs.list, packed.data(), packed.size() * sizeof(Packed), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 1;
}

// CHECK_IMG and CHECK_CTX for the shared frames below, which name the entry point they serve
static int check_img(const musica_ctx* c, const char* fn, uint32_t idx) {
    return (int)idx >= c->B ? fail("%s: image_index %u >= batch %d", fn, (unsigned)idx, c->B) : 1;
}
static int check_ctx(const musica_ctx* c, const char* fn) { return hipSetDevice(c->p.device) != hipSuccess ? fail("%s: hipSetDevice failed", fn) : 1; }

// The three list measurements (musica_sim_details / _edges / _gratings), in the manner of sim_derive_slot. `null`: the text of the
// call's NULL-argument refusal where an argument is NULL, else nullptr. list(side, packed, words): the call's *_check for the output
// plane (words: what its tables take). launch(a plane, a pitch, b plane, b pitch, list, results, tables). The results come back as
// `count` Result, the tables' `words` u32 into `tables`.
template <typename Packed, typename Result, typename List, typename Launch>
static int sim_patch_list(musica_ctx* c, const char* fn, const char* null, uint32_t idx, uint32_t slot, uint32_t count, const PatchBuffers<Packed>& bufs,
                          List list, Launch launch, Result* out, uint32_t* tables, uint64_t table_words) {
    if (!c) return fail("%s: ctx is NULL", fn);
    if (null) return fail("%s: %s is NULL", fn, null);
    if (c->N <= 2 * MUSICA_OUT_MARGIN) return fail("%s: image too small for the %d-pixel margin", fn, MUSICA_OUT_MARGIN);
    if (slot >= MUSICA_SIM_SLOTS) return fail("%s: slot %u >= %d", fn, slot, MUSICA_SIM_SLOTS);
    if (!c->study.written[slot]) return fail("%s: slot %u was never written", fn, slot);
    if (!check_img(c, fn, idx)) return 0;
    std::vector<Packed> packed;
    uint64_t words = 0;
    if (!list((int)sim_side(c), packed, words)) return 0;
    if (bufs.tables && table_words < words)
        return fail("%s: table_words %llu is less than the %llu words of the tables", fn, (unsigned long long)table_words, (unsigned long long)words);
    if (!check_ctx(c, fn)) return 0;
    StudyState& st = c->study;
    if (!(ensure(c, &(st.*bufs.out), bufs.most * bufs.out_words) && (!bufs.tables || ensure(c, &(st.*bufs.tables), bufs.tables_cap))))
        return fail("%s: device allocation failed", fn);
    if (!upload_list(c, fn, bufs, packed)) return 0;
    const int pitch = c->lv[0].pitch;
    uint32_t* d_tables = bufs.tables ? st.*bufs.tables : nullptr;
    launch(image_slice(c, c->d_graded, idx) + (size_t)MUSICA_OUT_MARGIN * pitch + MUSICA_OUT_MARGIN, pitch, st.slot[slot], (int)sim_side(c), st.*bufs.list,
           st.*bufs.out, d_tables);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(out, st.*bufs.out, (size_t)count * sizeof(Result), hipMemcpyDeviceToHost, c->stream));
    if (bufs.tables) HIP_OK(hipMemcpyAsync(tables, d_tables, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 1;
}

// Before an alteration writes into d_input: when the last step read d_input, keep it for the getters that recompute from the input.
static int alter_keep_input(musica_ctx* c, const char* fn) {
    if (c->cur_input != c->d_input) return 1;
    const size_t nn = (size_t)c->N * c->N;
    if (!ensure(c, &c->d_input_kept, (size_t)c->B * nn)) return fail("%s: device allocation failed", fn);
    HIP_OK(hipMemcpyAsync(c->d_input_kept, c->d_input, (size_t)c->B * nn * sizeof(uint16_t), hipMemcpyDeviceToDevice, c->stream));
    c->cur_input = c->d_input_kept;
    return 1;
}

// The alterations that have an entry point of their own, every one a launch from the source plane into image idx of the input buffer.
// `null`: the text of the call's NULL-argument refusal where an argument is NULL, else nullptr. check(): what the call refuses about
// its other arguments (1, or fail(...)), no device work. prepare(): its device buffers and uploads (1, or fail(...)). launch(src, dst).
template <typename Check, typename Prepare, typename Launch>
static int alter_into(musica_ctx* c, const char* fn, const char* null, uint32_t idx, Check check, Prepare prepare, Launch launch) {
    if (!c) return fail("%s: ctx is NULL", fn);
    if (null) return fail("%s: %s is NULL", fn, null);
    if (!c->study.d_alter_src) return fail("%s: no source plane (musica_alter_set_source)", fn);
    if (!check() || !check_img(c, fn, idx) || !check_ctx(c, fn) || !prepare() || !alter_keep_input(c, fn)) return 0;
    launch(c->study.d_alter_src, c->d_input + idx * (size_t)c->N * c->N);
    HIP_OK(hipGetLastError());
    return 1;
}
static int nothing() { return 1; }

// What musica_sim_compare and musica_sim_joint refuse, in the same words (`what`: the entry point), before any device work.
// musica_sim_profiles has no window: its smallest side is 1 (min_side) and its largest count max_count.
static int sim_check_queries(musica_ctx* c, const char* what, uint32_t count, const musica_sim_query* qs, const void* out, uint32_t min_side = 7,
                             uint32_t max_count = MUSICA_SIM_MAX_QUERIES) {
    if (!c) return fail("%s: ctx is NULL", what);
    if (!qs || !out) return fail("%s: queries or results is NULL", what);
    if (count == 0 || count > max_count) return fail("%s: count %u out of range [1, %u]", what, count, max_count);
    if (c->N <= 2 * MUSICA_OUT_MARGIN) return fail("%s: image too small for the %d-pixel margin", what, MUSICA_OUT_MARGIN);
    const uint64_t nw = sim_side(c);
    for (uint32_t i = 0; i < count; i++) {
        const musica_sim_query& q = qs[i];
        if (q.slot >= MUSICA_SIM_SLOTS) return fail("%s: query %u: slot %u >= %d", what, i, q.slot, MUSICA_SIM_SLOTS);
        if (!c->study.written[q.slot]) return fail("%s: query %u: slot %u was never written", what, i, q.slot);
        if ((int)q.image_index >= c->B) return fail("%s: query %u: image_index %u >= batch %d", what, i, q.image_index, c->B);
        if (min_side == 7 && (q.w < 7 || q.h < 7)) return fail("%s: query %u: region %u x %u is smaller than the 7 x 7 SSIM window", what, i, q.w, q.h);
        if (q.w < min_side || q.h < min_side) return fail("%s: query %u: region %u x %u has a side below %u", what, i, q.w, q.h, min_side);
        if ((uint64_t)q.ax + q.w > nw || (uint64_t)q.ay + q.h > nw || (uint64_t)q.bx + q.w > nw || (uint64_t)q.by + q.h > nw)
            return fail("%s: query %u: region (%u, %u) / (%u, %u) + %u x %u leaves the %llu x %llu planes", what, i, q.ax, q.ay, q.bx, q.by,
                        q.w, q.h, (unsigned long long)nw, (unsigned long long)nw);
    }
    return 1;
}

// Where a query's two regions lie: a in the graded plane of its image (margin included), b in its slot's plane.
static void sim_region(const musica_ctx* c, const musica_sim_query& q, SimRegion& d) {
    d.a = image_slice(c, c->d_graded, q.image_index) + (size_t)(q.ay + MUSICA_OUT_MARGIN) * c->lv[0].pitch + q.ax + MUSICA_OUT_MARGIN;
    d.b = c->study.slot[q.slot] + (size_t)q.by * sim_side(c) + q.bx;
    d.a_pitch = c->lv[0].pitch;
    d.b_pitch = (int)sim_side(c);
    d.w = (int)q.w;
    d.h = (int)q.h;
}

// ---- the table comparisons (musica_sim_profiles / _levels / _gradients / _order / _lattice / _blobs / _spectrum / _cooccurrence / _granulometry / _contours / _minkowski / _reach) -----------------------------------------------
// Where a table call keeps its queries and its flat tables in musica_ctx::study, and what it takes: at most `most` queries with sides
// of at least `min_side`. The tables' buffer holds `tables_cap` words from the first call on; where `grown` names its capacity it
// holds the words of the largest call so far instead.
template <typename QueryDev, typename Word>
struct TableBuffers {
    QueryDev* StudyState::*queries;
    Word* StudyState::*tables;
    uint32_t most, min_side;
    size_t tables_cap;
    size_t StudyState::*grown = nullptr;
};
constexpr TableBuffers<ProfileQueryDev, uint32_t> kProfileBuffers{&StudyState::d_profile_q, &StudyState::d_profile_tables, MUSICA_PROFILE_MAX_QUERIES, 1, 0, &StudyState::profile_tables_cap};
constexpr TableBuffers<LevelQueryDev, unsigned long long> kLevelBuffers{&StudyState::d_level_q, &StudyState::d_level_tables, MUSICA_LEVEL_MAX_QUERIES, 1, (size_t)MUSICA_LEVEL_MAX_QUERIES * kLevelMaxClasses * kLevelWords};
constexpr TableBuffers<GradQueryDev, unsigned long long> kGradBuffers{&StudyState::d_grad_q, &StudyState::d_grad_tables, MUSICA_SIM_MAX_QUERIES, 7, (size_t)MUSICA_SIM_MAX_QUERIES * kGradClasses * kGradWords};
constexpr TableBuffers<OrderQueryDev, unsigned long long> kOrderBuffers{&StudyState::d_order_q, &StudyState::d_order_tables, MUSICA_SIM_MAX_QUERIES, 7, (size_t)MUSICA_SIM_MAX_QUERIES * kOrderTableWords};
constexpr TableBuffers<LatticeQueryDev, unsigned long long> kLatticeBuffers{&StudyState::d_lattice_q, &StudyState::d_lattice_tables, MUSICA_LATTICE_MAX_QUERIES, 2, (size_t)MUSICA_LATTICE_MAX_QUERIES * kLatticeMaxPeriod * kLatticeMaxPeriod * kLatticeWords};
constexpr TableBuffers<BlobQueryDev, unsigned long long> kBlobBuffers{&StudyState::d_blob_q, &StudyState::d_blob_tables, MUSICA_BLOBS_MAX_QUERIES, 1, (size_t)MUSICA_BLOBS_MAX_QUERIES * kBlobClasses * kBlobWords};
constexpr TableBuffers<SpectrumQueryDev, unsigned long long> kSpectrumBuffers{&StudyState::d_spectrum_q, &StudyState::d_spectrum_tables, MUSICA_SPECTRUM_MAX_QUERIES, 1, (size_t)MUSICA_SPECTRUM_MAX_QUERIES * kSpectrumMaxTile * kSpectrumMaxTile * kSpectrumWords};
constexpr TableBuffers<CooccurrenceQueryDev, uint32_t> kCooccurrenceBuffers{&StudyState::d_cooccurrence_q, &StudyState::d_cooccurrence_tables, MUSICA_COOCCURRENCE_MAX_QUERIES, 1, (size_t)MUSICA_COOCCURRENCE_MAX_QUERIES * MUSICA_COOCCURRENCE_MAX_DISTANCES * 4 * 2 * kCooccurrenceMaxLevels * kCooccurrenceMaxLevels};
constexpr TableBuffers<GranulometryQueryDev, unsigned long long> kGranulometryBuffers{&StudyState::d_granulometry_q, &StudyState::d_granulometry_tables, MUSICA_GRANULOMETRY_MAX_QUERIES, 1, (size_t)MUSICA_GRANULOMETRY_MAX_QUERIES * (MUSICA_GRANULOMETRY_MAX_RADII + 1) * 2 * kGranulometryWords};
constexpr TableBuffers<ContourQueryDev, unsigned long long> kContourBuffers{&StudyState::d_contour_q, &StudyState::d_contour_tables, MUSICA_CONTOURS_MAX_QUERIES, 1, (size_t)MUSICA_CONTOURS_MAX_QUERIES * 2 * (MUSICA_CONTOURS_MAX_RADIUS * MUSICA_CONTOURS_MAX_RADIUS + 2)};
constexpr TableBuffers<MinkowskiQueryDev, uint32_t> kMinkowskiBuffers{&StudyState::d_minkowski_q, &StudyState::d_minkowski_tables, MUSICA_MINKOWSKI_MAX_QUERIES, 1, (size_t)MUSICA_MINKOWSKI_MAX_QUERIES * MUSICA_MINKOWSKI_SIDES * MUSICA_MINKOWSKI_KINDS * 256};
constexpr TableBuffers<ReachQueryDev, unsigned long long> kReachBuffers{&StudyState::d_reach_q, &StudyState::d_reach_tables, MUSICA_REACH_MAX_QUERIES, 1, (size_t)MUSICA_REACH_MAX_QUERIES * (MUSICA_REACH_MAX_RADII + 1) * kReachWords};

// What a call's place() says of one query: its tiles or chunks (the launch's grid.x is the largest) and the words of its table.
struct TablePlace {
    int units;
    size_t words;
};

// The query's grid of MUSICA_SIM_TILE^2 tiles over w x h pixels (its region, or the interior that the kernel tiles), and their number.
template <typename D>
static int tile_grid(D& d, uint32_t w, uint32_t h) {
    d.tiles_x = tiles_along(w);
    d.tiles_y = tiles_along(h);
    return d.tiles_x * d.tiles_y;
}

// The sum of column `col` of a table of `rows` rows of `stride` words: the ssd of a query from its table's sum_dd.
template <typename Word>
static uint64_t column_sum(const Word* t, size_t rows, size_t stride, size_t col) {
    uint64_t sum = 0;
    for (size_t k = 0; k < rows; k++) sum += t[k * stride + col];
    return sum;
}

// The five table calls, in the manner of sim_patch_list: sim_check_queries, then check() (the call's refusals about its other arguments:
// 1, or fail(...)), then the tables' refusals; no device work so far. place(q, d) fills what query q's device form d holds beyond its
// regions and its table's place (the tables lie one behind the other). prepare(): the call's other device buffers and what it enqueues
// before its launch; launch(queries, the largest units, tables) into zeroed tables; fetch(): what it copies back beside the tables (both
// 1, or fail(...)). One wait for the stream, then finish(i, q, t) fills out[i] behind its table_offset from query i's table t in `tables`.
template <typename QueryDev, typename Word, typename HostWord, typename Result, typename Check, typename Place, typename Prepare, typename Launch, typename Fetch, typename Finish>
static int sim_query_tables(musica_ctx* c, const char* fn, const TableBuffers<QueryDev, Word>& bufs, uint32_t count, const musica_sim_query* qs, Result* out,
                            HostWord* tables, uint64_t table_words, Check check, Place place, Prepare prepare, Launch launch, Fetch fetch, Finish finish) {
    static_assert(sizeof(HostWord) == sizeof(Word), "the tables come back as the device's words");
    if (!sim_check_queries(c, fn, count, qs, out, bufs.min_side, bufs.most) || !check()) return 0;
    if (!tables) return fail("%s: tables is NULL", fn);
    std::vector<QueryDev> hq(count);
    size_t words = 0;
    int max_units = 1;
    for (uint32_t i = 0; i < count; i++) {
        sim_region(c, qs[i], hq[i]);
        hq[i].table = words;
        const TablePlace at = place(qs[i], hq[i]);
        max_units = std::max(max_units, at.units);
        words += at.words;
    }
    if (table_words < words) return fail("%s: table_words %llu is less than the %llu words of the tables", fn, (unsigned long long)table_words, (unsigned long long)words);
    if (!check_ctx(c, fn)) return 0;
    StudyState& st = c->study;
    if (!(ensure(c, &(st.*bufs.queries), bufs.most) && (bufs.grown || ensure(c, &(st.*bufs.tables), bufs.tables_cap)))) return fail("%s: device allocation failed", fn);
    if (bufs.grown && !grow(c, fn, &(st.*bufs.tables), &(st.*bufs.grown), words, "table words")) return 0;
    if (!prepare()) return 0;
    HIP_OK(hipMemcpyAsync(st.*bufs.queries, hq.data(), count * sizeof(QueryDev), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemsetAsync(st.*bufs.tables, 0, words * sizeof(Word), c->stream));   // the workgroups add into them
    launch(st.*bufs.queries, max_units, st.*bufs.tables);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(tables, st.*bufs.tables, words * sizeof(Word), hipMemcpyDeviceToHost, c->stream));
    if (!fetch()) return 0;
    HIP_OK(hipStreamSynchronize(c->stream));   // hq, the tables and what fetch() copies are read by then
    for (uint32_t i = 0; i < count; i++) {
        out[i].table_offset = hq[i].table;
        finish(i, qs[i], tables + hq[i].table);
    }
    return 1;
}

// harness.ssim_similarity: c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2 (float ** is C pow); cov_norm = npx / (npx - 1)
static SimConsts sim_consts() {
    const double k1 = 0.01 * 255, k2 = 0.03 * 255;
    return {pow(k1, 2.0), pow(k2, 2.0), 49.0 / 48.0};
}

extern "C" {

// ---- reference slots (musica_sim_*, include/musica.h) -------------------------------------------------------------------------------
int musica_sim_capture(musica_ctx* c, uint32_t slot, uint32_t idx) {
    if (!c) return fail("musica_sim_capture: ctx is NULL");
    if (slot >= MUSICA_SIM_SLOTS) return fail("musica_sim_capture: slot %u >= %d", slot, MUSICA_SIM_SLOTS);
    CHECK_IMG(c, idx);
    uint8_t* dst = sim_slot_for_write(c, "musica_sim_capture", slot);
    if (!dst) return 0;
    launch_out_pixels(c->stream, image_slice(c, c->d_graded, idx), c->lv[0], MUSICA_OUT_MARGIN, dst);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("musica_sim_capture: launch failed: %s", hipGetErrorString(e));
    c->study.written[slot] = true;
    return 1;
}

int musica_sim_set_reference(musica_ctx* c, uint32_t slot, const uint8_t* pixels) {
    if (!c) return fail("musica_sim_set_reference: ctx is NULL");
    if (!pixels) return fail("musica_sim_set_reference: pixels is NULL");
    if (slot >= MUSICA_SIM_SLOTS) return fail("musica_sim_set_reference: slot %u >= %d", slot, MUSICA_SIM_SLOTS);
    uint8_t* dst = sim_slot_for_write(c, "musica_sim_set_reference", slot);
    if (!dst) return 0;
    HIP_OK(hipMemcpyAsync(dst, pixels, sim_side(c) * sim_side(c), hipMemcpyHostToDevice, c->stream));   // after what the stream holds (a compare reading the slot)
    HIP_OK(hipStreamSynchronize(c->stream));                                                             // `pixels` is borrowed for the call
    c->study.written[slot] = true;
    return 1;
}

int musica_sim_set_vendor_reference(musica_ctx* c, uint32_t slot, const void* pixels, uint32_t bits_allocated) {
    if (!c) return fail("musica_sim_set_vendor_reference: ctx is NULL");
    if (!pixels) return fail("musica_sim_set_vendor_reference: pixels is NULL");
    if (slot >= MUSICA_SIM_SLOTS) return fail("musica_sim_set_vendor_reference: slot %u >= %d", slot, MUSICA_SIM_SLOTS);
    if (bits_allocated != 8 && bits_allocated != 16) return fail("musica_sim_set_vendor_reference: bits_allocated %u is neither 8 nor 16", bits_allocated);
    uint8_t* dst = sim_slot_for_write(c, "musica_sim_set_vendor_reference", slot);
    if (!dst) return 0;
    const size_t count = sim_side(c) * sim_side(c);
    if (!ensure(c, &c->study.d_vendor, count)) return fail("musica_sim_set_vendor_reference: device allocation of the staging plane failed");
    // after what the stream holds (a compare reading the slot); `pixels` is borrowed for the call
    HIP_OK(hipMemcpyAsync(c->study.d_vendor, pixels, count * (bits_allocated / 8), hipMemcpyHostToDevice, c->stream));
    launch_sim_vendor(c->stream, c->study.d_vendor, (int)bits_allocated, dst, (long long)count);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(c->stream));
    c->study.written[slot] = true;
    return 1;
}

int musica_sim_get_reference(musica_ctx* c, uint32_t slot, uint8_t* dst) {
    if (!c) return fail("musica_sim_get_reference: ctx is NULL");
    if (!dst) return fail("musica_sim_get_reference: dst is NULL");
    if (slot >= MUSICA_SIM_SLOTS) return fail("musica_sim_get_reference: slot %u >= %d", slot, MUSICA_SIM_SLOTS);
    if (!c->study.written[slot]) return fail("musica_sim_get_reference: slot %u was never written", slot);
    CHECK_CTX(c);
    const size_t nw = sim_side(c);
    HIP_OK(hipMemcpyAsync(dst, c->study.slot[slot], nw * nw, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 1;
}

static bool finite_all(const double* v, int n) {
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

int musica_sim_rotate_reference(musica_ctx* c, uint32_t dst_slot, uint32_t src_slot, const double matrix[4], const double offset[2]) {
    if (!c) return fail("musica_sim_rotate_reference: ctx is NULL");
    if (!matrix || !offset) return fail("musica_sim_rotate_reference: matrix or offset is NULL");
    return sim_derive_slot(
        c, "musica_sim_rotate_reference", dst_slot, src_slot,
        [&] { return finite_all(matrix, 4) && finite_all(offset, 2) ? 1 : fail("musica_sim_rotate_reference: matrix or offset is not finite"); },
        [&](const uint8_t* src, uint8_t* dst) {
            AlterDev a{};
            a.n = (int)sim_side(c);
            memcpy(a.m, matrix, sizeof(a.m));
            memcpy(a.off, offset, sizeof(a.off));
            launch_rotate_u8(c->stream, src, dst, a);
        });
}

int musica_sim_transform_reference(musica_ctx* c, uint32_t dst_slot, uint32_t src_slot, uint32_t element) {
    if (!c) return fail("musica_sim_transform_reference: ctx is NULL");
    return sim_derive_slot(
        c, "musica_sim_transform_reference", dst_slot, src_slot,
        [&] { return element <= 7 ? 1 : fail("musica_sim_transform_reference: element %u is not one of the square's 8 symmetries (0 .. 7)", element); },
        [&](const uint8_t* src, uint8_t* dst) { launch_symmetry_u8(c->stream, src, dst, (int)sim_side(c), (int)element); });
}

static_assert(kBlurMaxRadius == MUSICA_BLUR_MAX_RADIUS, "kernels_blur.hip instantiates the radii of include/musica.h");

int musica_sim_blur_reference(musica_ctx* c, uint32_t dst_slot, uint32_t src_slot, uint32_t radius) {
    if (!c) return fail("musica_sim_blur_reference: ctx is NULL");
    return sim_derive_slot(
        c, "musica_sim_blur_reference", dst_slot, src_slot,
        [&] { return radius >= 1 && radius <= MUSICA_BLUR_MAX_RADIUS ? 1 : fail("musica_sim_blur_reference: radius %u out of range [1, %d]", radius, MUSICA_BLUR_MAX_RADIUS); },
        [&](const uint8_t* src, uint8_t* dst) { launch_blur_u8(c->stream, src, dst, (int)sim_side(c), (int)radius); });
}

int musica_sim_codec_reference(musica_ctx* c, uint32_t dst_slot, uint32_t src_slot, const uint16_t table[64], uint32_t origin) {
    if (!c) return fail("musica_sim_codec_reference: ctx is NULL");
    if (!table) return fail("musica_sim_codec_reference: table is NULL");
    CodecTable t;
    return sim_derive_slot(
        c, "musica_sim_codec_reference", dst_slot, src_slot, [&] { return codec_check("musica_sim_codec_reference", table, origin, t); },
        [&](const uint8_t* src, uint8_t* dst) { launch_codec_u8(c->stream, src, dst, (int)sim_side(c), (int)origin, t); });
}

int musica_sim_zoom_reference(musica_ctx* c, uint32_t dst_slot, uint32_t src_slot, uint32_t p, uint32_t q) {
    if (!c) return fail("musica_sim_zoom_reference: ctx is NULL");
    if (!zoom_check("musica_sim_zoom_reference", p, q)) return 0;
    return sim_derive_slot(
        c, "musica_sim_zoom_reference", dst_slot, src_slot, [] { return 1; },   // nothing more to refuse
        [&](const uint8_t* src, uint8_t* dst) { launch_zoom_u8(c->stream, src, dst, (int)sim_side(c), (int)p, (int)q); });
}

int musica_sim_scatter_reference(musica_ctx* c, uint32_t dst_slot, uint32_t src_slot, uint32_t radius, uint32_t num, uint32_t den) {
    if (!c) return fail("musica_sim_scatter_reference: ctx is NULL");
    if (!scatter_check("musica_sim_scatter_reference", radius, num, den)) return 0;
    return sim_derive_slot(
        c, "musica_sim_scatter_reference", dst_slot, src_slot,
        [&] { return hipSetDevice(c->p.device) == hipSuccess ? scatter_plane(c, "musica_sim_scatter_reference") : fail("musica_sim_scatter_reference: hipSetDevice failed"); },
        [&](const uint8_t* src, uint8_t* dst) {
            launch_scatter_u8(c->stream, src, dst, c->study.d_scatter, (int)sim_side(c), (int)radius, (int)num, (int)den);
        });
}

int musica_sim_warp_reference(musica_ctx* c, uint32_t dst_slot, uint32_t src_slot, const int16_t* field, uint32_t nodes, uint32_t origin) {
    ABI_TRY
    if (!c) return fail("musica_sim_warp_reference: ctx is NULL");
    if (!field) return fail("musica_sim_warp_reference: field is NULL");
    std::vector<uint32_t> packed;
    int m = 0;
    return sim_derive_slot(
        c, "musica_sim_warp_reference", dst_slot, src_slot,
        [&] {   // behind the slot rules: a written source implies a plane
            if (!warp_check("musica_sim_warp_reference", field, nodes, origin, sim_side(c), packed, &m)) return 0;
            if (hipSetDevice(c->p.device) != hipSuccess) return fail("musica_sim_warp_reference: hipSetDevice failed");
            return warp_upload(c, "musica_sim_warp_reference", packed);
        },
        [&](const uint8_t* src, uint8_t* dst) { launch_warp_u8(c->stream, src, dst, (int)sim_side(c), c->study.d_warp_nodes, m, (int)origin); });   // kernels_warp.hip
    ABI_CATCH("musica_sim_warp_reference")
}

int musica_sim_remap_reference(musica_ctx* c, uint32_t dst_slot, uint32_t src_slot, const uint8_t lut[256]) {
    if (!c) return fail("musica_sim_remap_reference: ctx is NULL");
    if (!lut) return fail("musica_sim_remap_reference: lut is NULL");
    return sim_derive_slot(
        c, "musica_sim_remap_reference", dst_slot, src_slot, [] { return 1; },   // nothing more to refuse
        [&](const uint8_t* src, uint8_t* dst) {
            RemapLut t;
            memcpy(t.v, lut, sizeof(t.v));   // travels as a kernel argument: `lut` is free again when the call returns
            launch_sim_remap(c->stream, src, dst, t, (long long)(sim_side(c) * sim_side(c)));
        });
}

// ---- the query calls (musica_sim_compare / _joint / _displace / _multiscale) ----------------------------------------------------------------------
// harness.hist_similarity from the exact value counts: np.histogram(v, bins=256) of u8 data spans [lo, hi] = [min, max] and puts v
// into bin min(255, (v - lo) * 256 // (hi - lo)) — exactly, for every (lo, hi) — and everything into bin 128 when lo == hi
// (numpy widens the range by +-0.5).
static void sim_bins(const uint32_t* counts, uint32_t* bins, uint32_t* lo_out, uint32_t* hi_out) {
    int lo = 0, hi = 255;
    while (lo < 255 && counts[lo] == 0) lo++;
    while (hi > 0 && counts[hi] == 0) hi--;
    memset(bins, 0, 256 * sizeof(uint32_t));
    for (int v = lo; v <= hi; v++) {
        if (!counts[v]) continue;
        const int b = hi == lo ? 128 : std::min(255, (v - lo) * 256 / (hi - lo));
        bins[b] += counts[v];
    }
    *lo_out = (uint32_t)lo;
    *hi_out = (uint32_t)hi;
}

static void sim_finish(const uint32_t* counts /* a 256 | b 256 */, const SimPart& r, const musica_sim_query& q, musica_sim_result* o) {
    const uint64_t n = (uint64_t)q.w * q.h;
    o->sq_diff_sum = r.ssd;
    o->pixels = n;
    sim_bins(counts, o->bins_a, &o->min_a, &o->max_a);
    sim_bins(counts + 256, o->bins_b, &o->min_b, &o->max_b);
    o->mse = 1.0 - sqrt((double)r.ssd / (65025.0 * (double)n));                 // 1 - sqrt(mean(((a - b) / 255)^2))
    o->ssim = r.ssim / ((double)(q.w - 6) * (double)(q.h - 6));                // mean over the interior (borders of 3 cropped)
    uint64_t inter = 0;
    double e2 = 0.0, bc = 0.0;
    for (int i = 0; i < 256; i++) {
        inter += std::min(o->bins_a[i], o->bins_b[i]);
        const double na = (double)o->bins_a[i] / (double)n, nb = (double)o->bins_b[i] / (double)n;
        e2 += (na - nb) * (na - nb);
        bc += sqrt(na * nb);
    }
    o->hist_intersection = (double)inter / (double)n;
    o->hist_distance = sqrt(e2) / sqrt(2.0);
    o->hist_bhattacharyya = bc;
}

int musica_sim_compare(musica_ctx* c, uint32_t count, const musica_sim_query* qs, musica_sim_result* out) {
    ABI_TRY
    if (!sim_check_queries(c, "musica_sim_compare", count, qs, out)) return 0;
    CHECK_CTX(c);
    StudyState& st = c->study;
    if (!(ensure(c, &st.d_sim_q, MUSICA_SIM_MAX_QUERIES) && ensure(c, &st.d_sim_part, (size_t)MUSICA_SIM_MAX_QUERIES * kSimMaxBlocks) &&
          ensure(c, &st.d_sim_out, MUSICA_SIM_MAX_QUERIES) && ensure(c, &st.d_sim_hist, (size_t)MUSICA_SIM_MAX_QUERIES * 512)))
        return fail("musica_sim_compare: device allocation failed");
    std::vector<SimQueryDev> hq(count);
    int max_blocks = 1;
    for (uint32_t i = 0; i < count; i++) {
        sim_region(c, qs[i], hq[i]);
        sim_geometry(hq[i]);
        max_blocks = std::max(max_blocks, hq[i].strips * hq[i].segs);
    }
    HIP_OK(hipMemcpyAsync(st.d_sim_q, hq.data(), count * sizeof(SimQueryDev), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemsetAsync(st.d_sim_hist, 0, (size_t)count * 512 * sizeof(uint32_t), c->stream));
    launch_sim(c->stream, st.d_sim_q, (int)count, max_blocks, st.d_sim_part, st.d_sim_hist, st.d_sim_out, sim_consts());
    HIP_OK(hipGetLastError());
    std::vector<uint32_t> hist((size_t)count * 512);
    std::vector<SimPart> parts(count);
    HIP_OK(hipMemcpyAsync(hist.data(), st.d_sim_hist, hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(parts.data(), st.d_sim_out, count * sizeof(SimPart), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));   // hq and the results are read by then
    for (uint32_t i = 0; i < count; i++) sim_finish(hist.data() + (size_t)i * 512, parts[i], qs[i], out + i);
    return 1;
    ABI_CATCH("musica_sim_compare")
}

// musica_sim_joint's numbers from one exact table (include/musica.h states them; harness.tone_similarities restates them): sums in
// ascending a, then ascending b, zero counts skipped; the variance numerators as exact 128-bit integers, one f64 division per term.
static void joint_finish(const uint32_t* J, const musica_sim_query& q, musica_sim_joint_result* o) {
    typedef unsigned __int128 u128;
    const uint64_t n = (uint64_t)q.w * q.h;
    const double dn = (double)n;
    uint64_t A[256] = {}, B[256] = {}, S[256] = {}, Q[256] = {};
    uint64_t ssd = 0;
    for (int a = 0; a < 256; a++)
        for (int b = 0; b < 256; b++) {
            const uint64_t j = J[a * 256 + b];
            if (!j) continue;
            A[a] += j;
            B[b] += j;
            S[b] += (uint64_t)a * j;
            Q[b] += (uint64_t)(a * a) * j;
            ssd += (uint64_t)((a - b) * (a - b)) * j;
        }
    double h_a = 0.0, h_b = 0.0, h_ab = 0.0, mi = 0.0;
    for (int a = 0; a < 256; a++)
        if (A[a]) { const double p = (double)A[a] / dn; h_a -= p * log(p); }
    for (int b = 0; b < 256; b++)
        if (B[b]) { const double p = (double)B[b] / dn; h_b -= p * log(p); }
    for (int a = 0; a < 256; a++)
        for (int b = 0; b < 256; b++) {
            const uint64_t j = J[a * 256 + b];
            if (!j) continue;
            const double p = (double)j / dn;
            h_ab -= p * log(p);
            mi += p * log((double)(j * n) / (double)(A[a] * B[b]));   // both products < 2^57
        }
    double ssw = 0.0;
    for (int b = 0; b < 256; b++) {
        o->tone_lut[b] = (uint8_t)(B[b] ? (2 * S[b] + B[b]) / (2 * B[b]) : (uint64_t)b);
        if (B[b]) ssw += (double)((u128)B[b] * Q[b] - (u128)S[b] * S[b]) / (double)B[b];   // B Q >= S^2 (Cauchy-Schwarz)
    }
    uint64_t sa = 0, saa = 0;
    for (int a = 0; a < 256; a++) {
        sa += (uint64_t)a * A[a];
        saa += (uint64_t)(a * a) * A[a];
    }
    const u128 sst_num = (u128)n * saa - (u128)sa * sa;
    o->mi = mi;
    o->nmi = h_a + h_b == 0.0 ? 1.0 : 2.0 * mi / (h_a + h_b);
    o->corr_ratio = sst_num == 0 ? 1.0 : 1.0 - ssw / ((double)sst_num / dn);
    o->tone_mse = 1.0 - sqrt(ssw / dn) / 255.0;
    o->h_a = h_a;
    o->h_b = h_b;
    o->h_ab = h_ab;
    o->pixels = n;
    o->sq_diff_sum = ssd;
}

int musica_sim_joint(musica_ctx* c, uint32_t count, const musica_sim_query* qs, musica_sim_joint_result* out, uint32_t* joint) {
    ABI_TRY
    if (!sim_check_queries(c, "musica_sim_joint", count, qs, out)) return 0;
    CHECK_CTX(c);
    StudyState& st = c->study;
    if (!(ensure(c, &st.d_joint_q, MUSICA_SIM_MAX_QUERIES) && ensure(c, &st.d_joint, (size_t)MUSICA_SIM_MAX_QUERIES * 65536)))
        return fail("musica_sim_joint: device allocation failed");
    std::vector<JointQueryDev> hq(count);
    int max_chunks = 1;
    for (uint32_t i = 0; i < count; i++) {
        sim_region(c, qs[i], hq[i]);
        joint_geometry(hq[i], (int)count);
        max_chunks = std::max(max_chunks, hq[i].chunks);
    }
    std::vector<uint32_t> own;
    if (!joint) {
        own.resize((size_t)count * 65536);
        joint = own.data();
    }
    HIP_OK(hipMemcpyAsync(st.d_joint_q, hq.data(), count * sizeof(JointQueryDev), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemsetAsync(st.d_joint, 0, (size_t)count * 65536 * sizeof(uint32_t), c->stream));
    launch_joint(c->stream, st.d_joint_q, (int)count, max_chunks, st.d_joint);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(joint, st.d_joint, (size_t)count * 65536 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));   // hq and the tables are read by then
    for (uint32_t i = 0; i < count; i++) {
        memset(out + i, 0, sizeof(out[i]));
        joint_finish(joint + (size_t)i * 65536, qs[i], out + i);
    }
    return 1;
    ABI_CATCH("musica_sim_joint")
}

// The argmin of an S x S displacement table by include/musica.h's tie rule: smallest value, then smallest dx^2 + dy^2, then smallest dy,
// then smallest dx (harness.displacement_from_table restates it).
static void displace_finish(const uint64_t* T, int radius, musica_sim_displace_result* o) {
    const int S = 2 * radius + 1;
    int by = radius, bx = radius;
    for (int y = 0; y < S; y++)
        for (int x = 0; x < S; x++) {
            const uint64_t v = T[y * S + x], m = T[by * S + bx];
            const int d2 = (x - radius) * (x - radius) + (y - radius) * (y - radius);
            const int m2 = (bx - radius) * (bx - radius) + (by - radius) * (by - radius);
            if (v < m || (v == m && d2 < m2)) {   // equal value and distance: the scan order is ascending dy, then ascending dx
                by = y;
                bx = x;
            }
        }
    o->ssd_zero = T[radius * S + radius];
    o->ssd_min = T[by * S + bx];
    o->dx = bx - radius;
    o->dy = by - radius;
}

int musica_sim_displace(musica_ctx* c, uint32_t count, const musica_sim_query* qs, uint32_t radius, musica_sim_displace_result* out,
                        uint64_t* tables, uint32_t* tile_tables) {
    ABI_TRY
    if (!sim_check_queries(c, "musica_sim_displace", count, qs, out)) return 0;
    if (radius < 1 || radius > MUSICA_SIM_MAX_RADIUS) return fail("musica_sim_displace: radius %u out of range [1, %d]", radius, MUSICA_SIM_MAX_RADIUS);
    const uint64_t nw = sim_side(c);
    for (uint32_t i = 0; i < count; i++) {
        const musica_sim_query& q = qs[i];
        if (q.bx < radius || q.by < radius || (uint64_t)q.bx + q.w + radius > nw || (uint64_t)q.by + q.h + radius > nw)
            return fail("musica_sim_displace: query %u: the b window (%u, %u) + %u x %u grown by the radius %u leaves the %llu x %llu plane", i, q.bx,
                        q.by, q.w, q.h, radius, (unsigned long long)nw, (unsigned long long)nw);
    }
    const size_t S2 = (size_t)(2 * radius + 1) * (2 * radius + 1);
    std::vector<DisplaceQueryDev> hq(count);
    TileRun run;
    for (uint32_t i = 0; i < count; i++) {
        sim_region(c, qs[i], hq[i]);
        run.place(hq[i], S2);
    }
    const size_t tile_words = run.next;
    CHECK_CTX(c);
    StudyState& st = c->study;
    if (!(ensure(c, &st.d_disp_q, MUSICA_SIM_MAX_QUERIES) &&
          ensure(c, &st.d_disp_tables, (size_t)MUSICA_SIM_MAX_QUERIES * (2 * MUSICA_SIM_MAX_RADIUS + 1) * (2 * MUSICA_SIM_MAX_RADIUS + 1)) &&
          ensure(c, &st.d_disp_off, MUSICA_SIM_MAX_QUERIES)))
        return fail("musica_sim_displace: device allocation failed");
    if (!grow(c, "musica_sim_displace", &st.d_disp_tiles, &st.disp_tiles_cap, tile_words, "tile-table words")) return 0;
    HIP_OK(hipMemcpyAsync(st.d_disp_q, hq.data(), count * sizeof(DisplaceQueryDev), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemsetAsync(st.d_disp_tables, 0, count * S2 * sizeof(unsigned long long), c->stream));
    HIP_OK(hipMemsetAsync(st.d_disp_off, 0, count * sizeof(uint32_t), c->stream));
    launch_displace(c->stream, st.d_disp_q, (int)count, run.max_tiles, (int)radius, st.d_disp_tiles, st.d_disp_tables, st.d_disp_off);
    HIP_OK(hipGetLastError());
    std::vector<uint64_t> own;
    if (!tables) {
        own.resize(count * S2);
        tables = own.data();
    }
    std::vector<uint32_t> off(count);
    HIP_OK(hipMemcpyAsync(tables, st.d_disp_tables, count * S2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(off.data(), st.d_disp_off, count * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (tile_tables) HIP_OK(hipMemcpyAsync(tile_tables, st.d_disp_tiles, tile_words * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));   // hq and the tables are read by then
    for (uint32_t i = 0; i < count; i++) {
        memset(out + i, 0, sizeof(out[i]));
        out[i].pixels = (uint64_t)qs[i].w * qs[i].h;
        out[i].tiles_x = (uint32_t)hq[i].tiles_x;
        out[i].tiles_y = (uint32_t)hq[i].tiles_y;
        out[i].tiles_off = off[i];
        displace_finish(tables + (size_t)i * S2, (int)radius, out + i);
    }
    return 1;
    ABI_CATCH("musica_sim_displace")
}

// musica_sim_multiscale's numbers of one query from the folded sums (include/musica.h states them; harness.multiscale_similarities
// restates them): the means, mse per scale, and the product of powers in ascending s with C pow.
static void scales_finish(const ScaleOut* r, const musica_sim_query& q, uint32_t scales, musica_sim_scales_result* o) {
    static const double W[MUSICA_SIM_MAX_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};   // Wang, Simoncelli, Bovik 2003
    memset(o, 0, sizeof(*o));
    o->scales = scales;
    o->pixels = (uint64_t)q.w * q.h;
    double wsum = 0.0;
    for (uint32_t s = 0; s < scales; s++) wsum += W[s];
    double ms = 1.0;
    for (uint32_t s = 0; s < scales; s++) {
        const uint64_t ws = q.w >> s, hs = q.h >> s;
        const double windows = (double)((ws - 6) * (hs - 6));
        o->plane_w[s] = (uint32_t)ws;
        o->plane_h[s] = (uint32_t)hs;
        o->ssim[s] = r[s].ssim / windows;
        o->cs[s] = r[s].cs / windows;
        o->lum[s] = r[s].lum / windows;
        o->ssd[s] = r[s].ssd;
        o->mse[s] = 1.0 - sqrt((double)r[s].ssd / (double)(hs * ws)) / (double)(255ull << (2 * s));
        ms *= pow(std::max(s + 1 < scales ? o->cs[s] : o->ssim[s], 0.0), W[s] / wsum);
    }
    o->ms_ssim = ms;
}

int musica_sim_multiscale(musica_ctx* c, uint32_t count, const musica_sim_query* qs, uint32_t scales, musica_sim_scales_result* out) {
    ABI_TRY
    if (!sim_check_queries(c, "musica_sim_multiscale", count, qs, out)) return 0;
    if (scales < 1 || scales > MUSICA_SIM_MAX_SCALES) return fail("musica_sim_multiscale: scales %u out of range [1, %d]", scales, MUSICA_SIM_MAX_SCALES);
    for (uint32_t i = 0; i < count; i++)
        if ((std::min(qs[i].w, qs[i].h) >> (scales - 1)) < 7)
            return fail("musica_sim_multiscale: query %u: region %u x %u is smaller than the 7 x 7 window at scale %u", i, qs[i].w, qs[i].h, scales - 1);
    std::vector<ScalePoolDev> hq(count);
    std::vector<ScaleJobDev> jobs((size_t)count * scales);
    size_t bytes = 0, tiles = 0;
    int max_tiles = 1, max_blocks = 1;
    for (uint32_t i = 0; i < count; i++) {
        ScalePoolDev& d = hq[i];
        sim_region(c, qs[i], d);
        d.scales = (int)scales;
        d.tiles_x = (d.w + kScalePoolW - 1) / kScalePoolW;
        d.tiles_y = (d.h + kScalePoolH - 1) / kScalePoolH;
        d.part_base = tiles;
        tiles += (size_t)d.tiles_x * d.tiles_y;
        max_tiles = std::max(max_tiles, d.tiles_x * d.tiles_y);
        for (uint32_t s = 0; s < MUSICA_SIM_MAX_SCALES; s++) d.plane_off[s] = 0;
        for (uint32_t s = 0; s < scales; s++) {
            ScaleJobDev& j = jobs[(size_t)i * scales + s];
            j.plane_off = d.plane_off[s] = bytes;
            j.w = d.w >> s;
            j.h = d.h >> s;
            j.scale = (int)s;
            j.query = (int)i;
            scales_geometry(j);
            max_blocks = std::max(max_blocks, j.strips * j.segs);
            bytes += ((size_t)j.w * j.h * (s == 0 ? 2 : 4) + 15) & ~(size_t)15;
        }
    }
    CHECK_CTX(c);
    StudyState& st = c->study;
    const size_t max_jobs = (size_t)MUSICA_SIM_MAX_QUERIES * MUSICA_SIM_MAX_SCALES;
    if (!(ensure(c, &st.d_scale_q, MUSICA_SIM_MAX_QUERIES) && ensure(c, &st.d_scale_jobs, max_jobs) &&
          ensure(c, &st.d_scale_part, max_jobs * kScaleMaxBlocks) && ensure(c, &st.d_scale_out, max_jobs)))
        return fail("musica_sim_multiscale: device allocation failed");
    if (!grow(c, "musica_sim_multiscale", &st.d_scale_planes, &st.scale_planes_cap, bytes) ||
        !grow(c, "musica_sim_multiscale", &st.d_scale_pool, &st.scale_pool_cap, tiles))
        return 0;
    ScaleConsts k;
    static_cast<SimConsts&>(k) = sim_consts();
    for (int s = 0; s < MUSICA_SIM_MAX_SCALES; s++) {
        k.div1[s] = (double)(49ull << (2 * s));   // 49 * 4^s and 49 * 16^s: exact doubles
        k.div2[s] = (double)(49ull << (4 * s));
    }
    HIP_OK(hipMemcpyAsync(st.d_scale_q, hq.data(), count * sizeof(ScalePoolDev), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(st.d_scale_jobs, jobs.data(), jobs.size() * sizeof(ScaleJobDev), hipMemcpyHostToDevice, c->stream));
    launch_scales(c->stream, st.d_scale_q, (int)count, max_tiles, st.d_scale_jobs, (int)jobs.size(), max_blocks, st.d_scale_planes, st.d_scale_pool,
                  st.d_scale_part, st.d_scale_out, k);
    HIP_OK(hipGetLastError());
    std::vector<ScaleOut> res(jobs.size());
    HIP_OK(hipMemcpyAsync(res.data(), st.d_scale_out, res.size() * sizeof(ScaleOut), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));   // hq, jobs and the results are read by then
    for (uint32_t i = 0; i < count; i++) scales_finish(res.data() + (size_t)i * scales, qs[i], scales, out + i);
    return 1;
    ABI_CATCH("musica_sim_multiscale")
}

// ---- the list measurements (musica_sim_details / _edges / _gratings / _points, include/musica.h; kernels_details.hip, kernels_edges.hip, kernels_gratings.hip, kernels_points.hip)
int musica_sim_details(musica_ctx* c, uint32_t idx, uint32_t slot, uint32_t count, const musica_detail* details, musica_sim_detail_result* out) {
    ABI_TRY
    return sim_patch_list(
        c, "musica_sim_details", !details || !out ? "details or results" : nullptr, idx, slot, count, kDetailBuffers,
        [&](int n, std::vector<PackedDetail>& packed, uint64_t&) { return details_check("musica_sim_details", count, details, n, false, packed); },
        [&](const float* a, int a_pitch, const uint8_t* b, int b_pitch, const PackedDetail* list, unsigned long long* results, uint32_t*) {
            launch_sim_details(c->stream, a, a_pitch, b, b_pitch, list, (int)count, results);
        },
        out, nullptr, 0);
    ABI_CATCH("musica_sim_details")
}

int musica_sim_edges(musica_ctx* c, uint32_t idx, uint32_t slot, uint32_t count, const musica_edge* edges, musica_sim_edge_result* out, uint32_t* tables,
                     uint64_t table_words) {
    ABI_TRY
    return sim_patch_list(
        c, "musica_sim_edges", !edges || !out || !tables ? "edges, results or tables" : nullptr, idx, slot, count, kEdgeBuffers,
        [&](int n, std::vector<PackedEdge>& packed, uint64_t& words) { return edges_check("musica_sim_edges", count, edges, n, false, packed, &words); },
        [&](const float* a, int a_pitch, const uint8_t* b, int b_pitch, const PackedEdge* list, unsigned long long* results, uint32_t* d_tables) {
            launch_sim_edges(c->stream, a, a_pitch, b, b_pitch, list, (int)count, results, d_tables);
        },
        out, tables, table_words);
    ABI_CATCH("musica_sim_edges")
}

int musica_sim_gratings(musica_ctx* c, uint32_t idx, uint32_t slot, uint32_t count, const musica_grating* gratings, musica_sim_grating_result* out,
                        uint32_t* tables, uint64_t table_words) {
    ABI_TRY
    return sim_patch_list(
        c, "musica_sim_gratings", !gratings || !out || !tables ? "gratings, results or tables" : nullptr, idx, slot, count, kGratingBuffers,
        [&](int n, std::vector<PackedGrating>& packed, uint64_t& words) {
            uint64_t periods = 0;
            const int ok = gratings_check("musica_sim_gratings", count, gratings, n, packed, &periods);
            words = 4 * periods;
            return ok;
        },
        [&](const float* a, int a_pitch, const uint8_t* b, int b_pitch, const PackedGrating* list, unsigned long long* results, uint32_t* d_tables) {
            launch_sim_gratings(c->stream, a, a_pitch, b, b_pitch, list, (int)count, results, d_tables);
        },
        out, tables, table_words);
    ABI_CATCH("musica_sim_gratings")
}

int musica_sim_points(musica_ctx* c, uint32_t idx, uint32_t slot, uint32_t count, const musica_defect* points, uint32_t groups, musica_sim_point_result* out,
                      uint32_t* tables, uint64_t table_words) {
    ABI_TRY
    std::vector<uint32_t> plan;   // lives until sim_patch_list has waited for the stream
    int chunks = 0;
    return sim_patch_list(
        c, "musica_sim_points", !points || !out || !tables ? "points, results or tables" : nullptr, idx, slot, count, kPointBuffers,
        [&](int n, std::vector<PackedPoint>& packed, uint64_t& words) {
            if (!points_check("musica_sim_points", count, points, n, false, groups, packed)) return 0;
            const uint64_t side = 2ull * points[0].radius + 1;
            words = groups * 3ull * side * side;
            chunks = point_plan(packed.data(), (int)count, plan);
            return 1;
        },
        [&](const float* a, int a_pitch, const uint8_t* b, int b_pitch, const PackedPoint* list, unsigned long long* results, uint32_t* d_tables) {
            launch_sim_points(c->stream, a, a_pitch, b, b_pitch, list, (int)count, (int)points[0].radius, (int)groups, plan.data(), chunks,
                              d_tables + kPointTableWords, results, d_tables);
        },
        out, tables, table_words);
    ABI_CATCH("musica_sim_points")
}

// ---- the channel responses of patches (musica_sim_observer, include/musica.h; kernels_observer.hip) ---------------------------------------
static_assert(kObserverMaxViews == MUSICA_OBSERVER_MAX_VIEWS && kObserverMaxBanks == MUSICA_OBSERVER_MAX_BANKS && kObserverMaxChannels == MUSICA_OBSERVER_MAX_CHANNELS &&
                  kObserverMaxHalf == MUSICA_OBSERVER_MAX_HALF,
              "kernels_observer.hip's u32 partials and int32 responses hold for the banks of include/musica.h");

// A plain body in sim_patch_list's order and words: that frame refuses windows that overlap, which views may, and carries one list.
int musica_sim_observer(musica_ctx* c, uint32_t idx, uint32_t slot, uint32_t bank_count, const musica_channel_bank* banks, uint32_t count, const musica_view* views,
                        musica_sim_observer_result* out, int32_t* tables, uint64_t table_words) {
    ABI_TRY
    const char* fn = "musica_sim_observer";
    if (!c) return fail("%s: ctx is NULL", fn);
    if (!banks || !views || !out || !tables) return fail("%s: banks, views, results or tables is NULL", fn);
    if (c->N <= 2 * MUSICA_OUT_MARGIN) return fail("%s: image too small for the %d-pixel margin", fn, MUSICA_OUT_MARGIN);
    if (slot >= MUSICA_SIM_SLOTS) return fail("%s: slot %u >= %d", fn, slot, MUSICA_SIM_SLOTS);
    if (!c->study.written[slot]) return fail("%s: slot %u was never written", fn, slot);
    if (!check_img(c, fn, idx)) return 0;
    if (bank_count == 0 || bank_count > MUSICA_OBSERVER_MAX_BANKS) return fail("%s: bank_count %u out of range [1, %d]", fn, bank_count, MUSICA_OBSERVER_MAX_BANKS);
    uint32_t max_channels = 0;
    for (uint32_t k = 0; k < bank_count; k++) {
        const musica_channel_bank& b = banks[k];
        if (!b.weights) return fail("%s: bank %u: weights is NULL", fn, k);
        if (b.half < 1 || b.half > MUSICA_OBSERVER_MAX_HALF) return fail("%s: bank %u: half %u out of range [1, %d]", fn, k, b.half, MUSICA_OBSERVER_MAX_HALF);
        if (b.channels < 1 || b.channels > MUSICA_OBSERVER_MAX_CHANNELS)
            return fail("%s: bank %u: channels %u out of range [1, %d]", fn, k, b.channels, MUSICA_OBSERVER_MAX_CHANNELS);
        max_channels = std::max(max_channels, b.channels);
    }
    if (count == 0 || count > MUSICA_OBSERVER_MAX_VIEWS) return fail("%s: count %u out of range [1, %d]", fn, count, MUSICA_OBSERVER_MAX_VIEWS);
    const int n = (int)sim_side(c);
    std::vector<PackedView> packed(count);
    uint64_t words = 0;
    for (uint32_t i = 0; i < count; i++) {
        const musica_view& v = views[i];
        if (v.bank >= bank_count) return fail("%s: view %u: bank %u is not below %u", fn, i, v.bank, bank_count);
        const int64_t r = banks[v.bank].half;
        if (v.x - r < 0 || v.y - r < 0 || v.x + r >= n || v.y + r >= n)
            return fail("%s: view %u: the window (%d, %d) +- %d leaves the %d x %d plane", fn, i, v.x, v.y, (int)r, n, n);
        packed[i] = {v.x, v.y, banks[v.bank].half, banks[v.bank].channels, 0u, (uint32_t)words};
        words += 2ull * banks[v.bank].channels;
    }
    if (table_words < words)
        return fail("%s: table_words %llu is less than the %llu words of the tables", fn, (unsigned long long)table_words, (unsigned long long)words);
    // the banks as the kernel reads them, one behind the other, once per call
    std::vector<uint32_t> weights;
    std::vector<uint32_t> bank_at(bank_count);
    for (uint32_t k = 0; k < bank_count; k++) {
        bank_at[k] = (uint32_t)weights.size();
        observer_pack(banks[k].weights, (int)banks[k].half, (int)banks[k].channels, weights);
    }
    for (uint32_t i = 0; i < count; i++) packed[i].weights = bank_at[views[i].bank];
    if (!check_ctx(c, fn)) return 0;
    StudyState& st = c->study;
    if (!(ensure(c, &st.d_obs_views, (size_t)MUSICA_OBSERVER_MAX_VIEWS) &&
          ensure(c, &st.d_obs_tables, (size_t)MUSICA_OBSERVER_MAX_VIEWS * 2 * MUSICA_OBSERVER_MAX_CHANNELS) &&
          ensure(c, &st.d_obs_sums, (size_t)MUSICA_OBSERVER_MAX_VIEWS * 2)))
        return fail("%s: device allocation failed", fn);
    if (!grow(c, fn, &st.d_obs_weights, &st.obs_weights_cap, weights.size(), "weight words")) return 0;
    // on the stream, behind the kernel that still reads the last call's
    HIP_OK(hipMemcpyAsync(st.d_obs_views, packed.data(), count * sizeof(PackedView), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(st.d_obs_weights, weights.data(), weights.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const int pitch = c->lv[0].pitch;
    launch_sim_observer(c->stream, image_slice(c, c->d_graded, idx) + (size_t)MUSICA_OUT_MARGIN * pitch + MUSICA_OUT_MARGIN, pitch, st.slot[slot], n, st.d_obs_views,
                        (int)count, (int)max_channels, st.d_obs_weights, st.d_obs_tables, st.d_obs_sums);
    HIP_OK(hipGetLastError());
    std::vector<uint32_t> sums(2 * (size_t)count);
    HIP_OK(hipMemcpyAsync(tables, st.d_obs_tables, (size_t)words * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(sums.data(), st.d_obs_sums, sums.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));   // packed, weights, the tables and the sums are read by then
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t side = 2 * packed[i].half + 1;
        out[i] = {packed[i].table, side * side, sums[2 * i], sums[2 * i + 1]};
    }
    return 1;
    ABI_CATCH("musica_sim_observer")
}

// ---- the profiles of a comparison (musica_sim_profiles, include/musica.h; kernels_gain.hip) ---------------------------------------------
static_assert(kProfileMaxQueries == MUSICA_PROFILE_MAX_QUERIES && kGainOne == MUSICA_GAIN_ONE, "kernels_gain.hip's limits are include/musica.h's");

int musica_sim_profiles(musica_ctx* c, uint32_t count, const musica_sim_query* qs, musica_sim_profile_result* out, uint32_t* tables, uint64_t table_words) {
    ABI_TRY
    return sim_query_tables(
        c, "musica_sim_profiles", kProfileBuffers, count, qs, out, tables, table_words, nothing,
        [](const musica_sim_query& q, ProfileQueryDev& d) { return TablePlace{tile_grid(d, q.w, q.h), 4 * ((size_t)q.w + q.h)}; }, nothing,
        [&](const ProfileQueryDev* d_qs, int max_tiles, uint32_t* d_tables) { launch_sim_profiles(c->stream, d_qs, (int)count, max_tiles, d_tables); }, nothing,
        [&](uint32_t i, const musica_sim_query& q, const uint32_t* t) {
            out[i].cols = q.w;
            out[i].rows = q.h;
            out[i].ssd = column_sum(t, q.w, 4, 2);   // the column table's sum_dd: every pixel once
            out[i].pixels = (uint64_t)q.w * q.h;
        });
    ABI_CATCH("musica_sim_profiles")
}

// ---- the levels of a comparison (musica_sim_levels, include/musica.h; kernels_levels.hip) -----------------------------------------------
static_assert(kLevelMaxQueries == MUSICA_LEVEL_MAX_QUERIES && kLevelMinShift == MUSICA_LEVEL_MIN_SHIFT && kLevelMaxShift == MUSICA_LEVEL_MAX_SHIFT &&
                  kLutEntries == MUSICA_LUT_ENTRIES && kLevelWords == MUSICA_LEVEL_WORDS,
              "kernels_levels.hip's limits are include/musica.h's");

int musica_sim_levels(musica_ctx* c, uint32_t shift, uint32_t count, const musica_sim_query* qs, musica_sim_level_result* out, uint64_t* tables, uint64_t table_words) {
    ABI_TRY
    size_t classes = 0;   // of a shift that check() has let through
    return sim_query_tables(
        c, "musica_sim_levels", kLevelBuffers, count, qs, out, tables, table_words,
        [&] {
            if (!c->study.d_alter_src) return fail("musica_sim_levels: no source plane (musica_alter_set_source)");
            if (shift < MUSICA_LEVEL_MIN_SHIFT || shift > MUSICA_LEVEL_MAX_SHIFT)
                return fail("musica_sim_levels: shift %u out of range [%d, %d]", shift, MUSICA_LEVEL_MIN_SHIFT, MUSICA_LEVEL_MAX_SHIFT);
            classes = (65535u >> shift) + 1;
            return 1;
        },
        [&](const musica_sim_query& q, LevelQueryDev& d) {
            d.s = c->study.d_alter_src + (size_t)(q.ay + MUSICA_OUT_MARGIN) * c->N + q.ax + MUSICA_OUT_MARGIN;   // the class is taken at side a's coordinates
            d.s_pitch = c->N;
            level_geometry(d, (int)count);
            return TablePlace{d.chunks, classes * kLevelWords};
        },
        nothing,
        [&](const LevelQueryDev* d_qs, int max_chunks, unsigned long long* d_tables) { launch_sim_levels(c->stream, d_qs, (int)count, max_chunks, (int)shift, d_tables); },
        nothing,
        [&](uint32_t i, const musica_sim_query& q, const uint64_t* t) {
            out[i].classes = classes;
            out[i].ssd = column_sum(t, classes, kLevelWords, 3);
            out[i].pixels = (uint64_t)q.w * q.h;
        });
    ABI_CATCH("musica_sim_levels")
}

// ---- the gradients of a comparison (musica_sim_gradients, include/musica.h; kernels_gradients.hip) --------------------------------------
static_assert(kGradClasses == MUSICA_GRADIENT_CLASSES && kGradWords == MUSICA_GRADIENT_WORDS && kGradC == MUSICA_GRADIENT_C,
              "kernels_gradients.hip's constants are include/musica.h's");

int musica_sim_gradients(musica_ctx* c, uint32_t count, const musica_sim_query* qs, musica_sim_gradient_result* out, uint64_t* tables, uint64_t table_words) {
    ABI_TRY
    size_t tiles = 0;
    std::vector<double> sums;   // lives until sim_query_tables has waited for the stream
    return sim_query_tables(
        c, "musica_sim_gradients", kGradBuffers, count, qs, out, tables, table_words, nothing,
        [&](const musica_sim_query& q, GradQueryDev& d) {
            d.tile_base = tiles;
            tiles += (size_t)tile_grid(d, q.w - 2, q.h - 2);   // of the interior
            return TablePlace{d.tiles_x * d.tiles_y, (size_t)kGradClasses * kGradWords};
        },
        [&] {
            if (!ensure(c, &c->study.d_grad_out, MUSICA_SIM_MAX_QUERIES)) return fail("musica_sim_gradients: device allocation failed");
            return grow(c, "musica_sim_gradients", &c->study.d_grad_part, &c->study.grad_part_cap, tiles, "tile partials");
        },
        [&](const GradQueryDev* d_qs, int max_tiles, unsigned long long* d_tables) { launch_sim_gradients(c->stream, d_qs, (int)count, max_tiles, d_tables, c->study.d_grad_part, c->study.d_grad_out); },
        [&] {
            sums.resize(count);
            HIP_OK(hipMemcpyAsync(sums.data(), c->study.d_grad_out, count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            return 1;
        },
        [&](uint32_t i, const musica_sim_query& q, const uint64_t*) {
            out[i].pixels = (uint64_t)(q.w - 2) * (q.h - 2);
            out[i].gsim = sums[i] / (double)out[i].pixels;
        });
    ABI_CATCH("musica_sim_gradients")
}

// ---- the local order of a comparison (musica_sim_order, include/musica.h; kernels_order.hip) --------------------------------------------
static_assert(kOrderRings == MUSICA_ORDER_RINGS && kOrderWords == MUSICA_ORDER_WORDS && kOrderBins == MUSICA_ORDER_BINS &&
                  kOrderTableWords == MUSICA_ORDER_TABLE_WORDS,
              "kernels_order.hip's constants are include/musica.h's");

int musica_sim_order(musica_ctx* c, uint32_t count, const musica_sim_query* qs, musica_sim_order_result* out, uint64_t* tables, uint64_t table_words) {
    ABI_TRY
    return sim_query_tables(
        c, "musica_sim_order", kOrderBuffers, count, qs, out, tables, table_words, nothing,
        [](const musica_sim_query& q, OrderQueryDev& d) { return TablePlace{tile_grid(d, q.w - 6, q.h - 6), (size_t)kOrderTableWords}; },   // of the interior
        nothing, [&](const OrderQueryDev* d_qs, int max_tiles, unsigned long long* d_tables) { launch_sim_order(c->stream, d_qs, (int)count, max_tiles, d_tables); },
        nothing,
        [&](uint32_t i, const musica_sim_query& q, const uint64_t*) {
            out[i].pixels = (uint64_t)(q.w - 6) * (q.h - 6);
        });
    ABI_CATCH("musica_sim_order")
}

// ---- the lattice sums of a comparison (musica_sim_lattice, include/musica.h; kernels_lattice.hip) --------------------------------------
static_assert(kLatticeWords == MUSICA_LATTICE_WORDS && kLatticeMaxPeriod == MUSICA_LATTICE_MAX_PERIOD && kLatticeMaxQueries == MUSICA_LATTICE_MAX_QUERIES, "kernels_lattice.hip's constants are include/musica.h's");

int musica_sim_lattice(musica_ctx* c, uint32_t period, uint32_t origin, uint32_t count, const musica_sim_query* qs, musica_sim_lattice_result* out, uint64_t* tables,
                       uint64_t table_words) {
    ABI_TRY
    size_t partials = 0;   // words of every query's partial tables
    return sim_query_tables(
        c, "musica_sim_lattice", kLatticeBuffers, count, qs, out, tables, table_words,
        [&] {
            if (period != 2 && period != 4 && period != 8 && period != 16 && period != 32) return fail("musica_sim_lattice: period %u is not one of 2, 4, 8, 16, 32", period);
            if (origin >= period) return fail("musica_sim_lattice: origin %u is not below the period %u", origin, period);
            return 1;
        },
        [&](const musica_sim_query& q, LatticeQueryDev& d) {   // of the counted pixels
            d.groups = lattice_groups(tile_grid(d, q.w - 1, q.h - 1), (int)period, env_int("MUSICA_LATTICE_GROUPS", 0));
            d.phase_x = (int)((q.ax + origin) % period);
            d.phase_y = (int)((q.ay + origin) % period);
            d.part = partials;
            partials += (size_t)d.groups * period * period * kLatticeWords;
            return TablePlace{d.groups, (size_t)period * period * kLatticeWords};
        },
        [&] { return grow(c, "musica_sim_lattice", &c->study.d_lattice_part, &c->study.lattice_part_cap, partials, "partial words"); },
        [&](const LatticeQueryDev* d_qs, int max_groups, unsigned long long* d_tables) {
            launch_sim_lattice(c->stream, d_qs, (int)count, max_groups, (int)period, c->study.d_lattice_part, d_tables);
        },
        nothing,
        [&](uint32_t i, const musica_sim_query& q, const uint64_t*) {
            out[i].pixels = (uint64_t)(q.w - 1) * (q.h - 1);
        });
    ABI_CATCH("musica_sim_lattice")
}

// ---- the connected components of a comparison's change mask (musica_sim_blobs, include/musica.h; kernels_blobs.hip) --------------------
static_assert(kBlobClasses == MUSICA_BLOB_CLASSES && kBlobWords == MUSICA_BLOB_WORDS && kBlobMaxQueries == MUSICA_BLOBS_MAX_QUERIES, "kernels_blobs.hip's constants are include/musica.h's");

int musica_sim_blobs(musica_ctx* c, uint32_t threshold, uint32_t connectivity, uint32_t count, const musica_sim_query* qs, musica_sim_blobs_result* out, uint64_t* tables,
                     uint64_t table_words, uint32_t* labels, uint64_t label_words) {
    ABI_TRY
    size_t pixels = 0, max_pixels = 0, tiles = 0;   // of the whole call: every query's w * h, the largest, every query's tiles
    BlobBest largest[kBlobMaxQueries];
    unsigned long long keys_err[kBlobMaxQueries + 1] = {};   // the keys, then the error word
    BlobScratch s = {};
    const int ok = sim_query_tables(
        c, "musica_sim_blobs", kBlobBuffers, count, qs, out, tables, table_words,
        [&] {
            if (threshold > 254) return fail("musica_sim_blobs: threshold %u is not in 0 .. 254", threshold);
            if (connectivity != 4 && connectivity != 8) return fail("musica_sim_blobs: connectivity %u is neither 4 nor 8", connectivity);
            uint64_t words = 0;
            for (uint32_t i = 0; i < count; i++) words += (uint64_t)qs[i].w * qs[i].h;
            if (labels && label_words < words)
                return fail("musica_sim_blobs: label_words %llu is less than the %llu words of the label planes", (unsigned long long)label_words, (unsigned long long)words);
            return 1;
        },
        [&](const musica_sim_query& q, BlobQueryDev& d) {
            const size_t n = (size_t)q.w * q.h;
            d.plane = pixels;
            d.tile0 = tiles;
            d.cap = (uint32_t)std::min<size_t>(n + 64, 0xFFFFFFFEu);
            d.pad = 0;
            pixels += n;
            max_pixels = std::max(max_pixels, n);
            const int own = tile_grid(d, q.w, q.h);
            tiles += (size_t)own;
            return TablePlace{own, (size_t)kBlobClasses * kBlobWords};
        },
        [&] {
            StudyState& st = c->study;
            if (!grow(c, "musica_sim_blobs", &st.d_blob_parent, &st.blob_plane_cap, pixels, "plane words", 1, &st.d_blob_slots) ||
                (labels && !grow(c, "musica_sim_blobs", &st.d_blob_labels, &st.blob_label_cap, pixels, "label words")) ||
                !grow(c, "musica_sim_blobs", &st.d_blob_recs, &st.blob_tile_cap, tiles, "tiles of records", kBlobTileRecords) ||
                !grow(c, "musica_sim_blobs", &st.d_blob_counts, &st.blob_count_cap, tiles, "tile counts"))
                return 0;
            if (!(ensure(c, &st.d_blob_best, (size_t)kBlobMaxQueries + 1) && ensure(c, &st.d_blob_largest, (size_t)kBlobMaxQueries)))
                return fail("musica_sim_blobs: device allocation failed");
            HIP_OK(hipMemsetAsync(st.d_blob_best, 0, sizeof(keys_err), c->stream));
            HIP_OK(hipMemsetAsync(st.d_blob_largest, 0, sizeof(largest), c->stream));
            s = BlobScratch{st.d_blob_parent, st.d_blob_slots, labels ? st.d_blob_labels : nullptr, st.d_blob_recs, st.d_blob_counts, st.d_blob_best, st.d_blob_largest,
                            reinterpret_cast<uint32_t*>(st.d_blob_best + kBlobMaxQueries)};
            return 1;
        },
        [&](const BlobQueryDev* d_qs, int max_tiles, unsigned long long* d_tables) {
            launch_sim_blobs(c->stream, d_qs, (int)count, max_tiles, max_pixels, (unsigned long long)tiles * kBlobTileRecords, threshold, (int)connectivity, s, d_tables);
        },
        [&] {
            HIP_OK(hipMemcpyAsync(keys_err, c->study.d_blob_best, sizeof(keys_err), hipMemcpyDeviceToHost, c->stream));
            HIP_OK(hipMemcpyAsync(largest, c->study.d_blob_largest, sizeof(largest), hipMemcpyDeviceToHost, c->stream));
            if (labels) HIP_OK(hipMemcpyAsync(labels, c->study.d_blob_labels, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            return 1;
        },
        [&](uint32_t i, const musica_sim_query& q, const uint64_t* t) {
            musica_sim_blobs_result& r = out[i];
            const BlobBest& b = largest[i];
            r.pixels = (uint64_t)q.w * q.h;
            r.changed = column_sum(t, kBlobClasses, kBlobWords, 1);
            r.components = column_sum(t, kBlobClasses, kBlobWords, 0);
            r.largest_n = b.n;
            r.largest_first = b.first;
            r.largest_x0 = b.x0;
            r.largest_y0 = b.y0;
            r.largest_x1 = b.x1;
            r.largest_y1 = b.y1;
            r.largest_sum_dd = b.sdd;
        });
    if (!ok) return 0;
    uint64_t at = 0;   // the label planes lie one behind the other, whether or not they were asked for
    for (uint32_t i = 0; i < count; i++) {
        out[i].label_offset = at;
        at += out[i].pixels;
    }
    if ((uint32_t)keys_err[kBlobMaxQueries])
        return fail("musica_sim_blobs: internal: a labelling loop hit its cap or a link did not descend (error word %u)", (uint32_t)keys_err[kBlobMaxQueries]);
    return 1;
    ABI_CATCH("musica_sim_blobs")
}

// ---- the Walsh spectrum of a comparison (musica_sim_spectrum, include/musica.h; kernels_spectrum.hip) ----------------------------------
static_assert(kSpectrumWords == MUSICA_SPECTRUM_WORDS && kSpectrumMaxTile == MUSICA_SPECTRUM_MAX_TILE && kSpectrumMaxQueries == MUSICA_SPECTRUM_MAX_QUERIES, "kernels_spectrum.hip's constants are include/musica.h's");

int musica_sim_spectrum(musica_ctx* c, uint32_t tile, uint32_t count, const musica_sim_query* qs, musica_sim_spectrum_result* out, int64_t* tables, uint64_t table_words) {
    ABI_TRY
    size_t partials = 0;   // words of every query's partial tables
    return sim_query_tables(
        c, "musica_sim_spectrum", kSpectrumBuffers, count, qs, out, tables, table_words,
        [&] {
            if (tile != 8 && tile != 16 && tile != 32 && tile != 64) return fail("musica_sim_spectrum: tile %u is not one of 8, 16, 32, 64", tile);
            return 1;
        },
        [&](const musica_sim_query& q, SpectrumQueryDev& d) {   // of the whole tiles
            d.tiled_w = (int)(q.w / tile * tile);
            d.tiled_h = (int)(q.h / tile * tile);
            const int blocks = tile_grid(d, (uint32_t)d.tiled_w, (uint32_t)d.tiled_h);   // 0 where either side holds no tile
            d.groups = spectrum_groups(blocks, env_int("MUSICA_SPECTRUM_GROUPS", 0));
            d.part = partials;
            partials += (size_t)d.groups * tile * tile * kSpectrumWords;
            return TablePlace{d.groups, (size_t)tile * tile * kSpectrumWords};
        },
        [&] { return grow(c, "musica_sim_spectrum", &c->study.d_spectrum_part, &c->study.spectrum_part_cap, partials, "partial words"); },
        [&](const SpectrumQueryDev* d_qs, int max_groups, unsigned long long* d_tables) {
            launch_sim_spectrum(c->stream, d_qs, (int)count, max_groups, (int)tile, c->study.d_spectrum_part, d_tables);
        },
        nothing,
        [&](uint32_t i, const musica_sim_query& q, const int64_t*) {
            out[i].tiles = (uint64_t)(q.w / tile) * (q.h / tile);
        });
    ABI_CATCH("musica_sim_spectrum")
}

// ---- the co-occurrence matrices of a comparison (musica_sim_cooccurrence, include/musica.h; kernels_cooccurrence.hip) ------------------
static_assert(kCooccurrenceMaxDistances == MUSICA_COOCCURRENCE_MAX_DISTANCES && kCooccurrenceMaxDistance == MUSICA_COOCCURRENCE_MAX_DISTANCE &&
                  kCooccurrenceMaxLevels == MUSICA_COOCCURRENCE_MAX_LEVELS && kCooccurrenceMaxQueries == MUSICA_COOCCURRENCE_MAX_QUERIES,
              "kernels_cooccurrence.hip's constants are include/musica.h's");

int musica_sim_cooccurrence(musica_ctx* c, uint32_t levels, uint32_t distance_count, const uint32_t* distances, uint32_t count, const musica_sim_query* qs,
                            musica_sim_cooccurrence_result* out, uint32_t* tables, uint64_t table_words) {
    ABI_TRY
    CooccurrenceDistances dist{};
    return sim_query_tables(
        c, "musica_sim_cooccurrence", kCooccurrenceBuffers, count, qs, out, tables, table_words,
        [&] {
            if (levels != 8 && levels != 16 && levels != 32 && levels != 64) return fail("musica_sim_cooccurrence: levels %u are not one of 8, 16, 32, 64", levels);
            if (!distances) return fail("musica_sim_cooccurrence: distances is NULL");
            if (distance_count == 0 || distance_count > MUSICA_COOCCURRENCE_MAX_DISTANCES)
                return fail("musica_sim_cooccurrence: distance_count %u out of range [1, %d]", distance_count, MUSICA_COOCCURRENCE_MAX_DISTANCES);
            for (uint32_t k = 0; k < distance_count; k++) {
                if (distances[k] < 1 || distances[k] > MUSICA_COOCCURRENCE_MAX_DISTANCE)
                    return fail("musica_sim_cooccurrence: distance %u: %u is not in 1 .. %d", k, distances[k], MUSICA_COOCCURRENCE_MAX_DISTANCE);
                if (k && distances[k] <= distances[k - 1])
                    return fail("musica_sim_cooccurrence: distance %u: %u is not above distance %u: %u", k, distances[k], k - 1, distances[k - 1]);
                dist.d[k] = (int)distances[k];
            }
            dist.count = (int)distance_count;
            return 1;
        },
        [&](const musica_sim_query& q, CooccurrenceQueryDev& d) {
            d.groups = cooccurrence_groups(tile_grid(d, q.w, q.h), env_int("MUSICA_COOCCURRENCE_GROUPS", 0));
            return TablePlace{d.groups, (size_t)distance_count * 4 * 2 * levels * levels};
        },
        nothing,
        [&](const CooccurrenceQueryDev* d_qs, int max_groups, uint32_t* d_tables) {
            launch_sim_cooccurrence(c->stream, d_qs, (int)count, max_groups, (int)levels, dist, d_tables);
        },
        nothing,
        [&](uint32_t i, const musica_sim_query& q, const uint32_t*) {
            memset(out[i].pairs, 0, sizeof(out[i].pairs));
            for (uint32_t k = 0; k < distance_count; k++) {
                const uint64_t d = distances[k], cols = q.w > d ? q.w - d : 0, rows = q.h > d ? q.h - d : 0;
                out[i].pairs[k][0] = cols * q.h;    // (d, 0)
                out[i].pairs[k][1] = cols * rows;   // (d, d)
                out[i].pairs[k][2] = q.w * rows;    // (0, d)
                out[i].pairs[k][3] = cols * rows;   // (-d, d)
            }
        });
    ABI_CATCH("musica_sim_cooccurrence")
}

// ---- the granulometry of a comparison (musica_sim_granulometry, include/musica.h; kernels_granulometry.hip) -----------------------------
static_assert(kGranulometryMaxRadii == MUSICA_GRANULOMETRY_MAX_RADII && kGranulometryMaxRadius == MUSICA_GRANULOMETRY_MAX_RADIUS &&
                  kGranulometryMaxQueries == MUSICA_GRANULOMETRY_MAX_QUERIES && kGranulometryWords == MUSICA_GRANULOMETRY_WORDS,
              "kernels_granulometry.hip's constants are include/musica.h's");

int musica_sim_granulometry(musica_ctx* c, uint32_t radius_count, const uint32_t* radii, uint32_t count, const musica_sim_query* qs,
                            musica_sim_granulometry_result* out, uint64_t* tables, uint64_t table_words) {
    ABI_TRY
    GranulometryRadii list{};
    return sim_query_tables(
        c, "musica_sim_granulometry", kGranulometryBuffers, count, qs, out, tables, table_words,
        [&] {
            if (!radii) return fail("musica_sim_granulometry: radii is NULL");
            if (radius_count == 0 || radius_count > MUSICA_GRANULOMETRY_MAX_RADII)
                return fail("musica_sim_granulometry: radius_count %u out of range [1, %d]", radius_count, MUSICA_GRANULOMETRY_MAX_RADII);
            for (uint32_t k = 0; k < radius_count; k++)
                if (radii[k] < 1 || radii[k] > MUSICA_GRANULOMETRY_MAX_RADIUS)
                    return fail("musica_sim_granulometry: radius %u: %u is not in 1 .. %d", k, radii[k], MUSICA_GRANULOMETRY_MAX_RADIUS);
            for (uint32_t k = 1; k < radius_count; k++)
                if (radii[k] <= radii[k - 1])
                    return fail("musica_sim_granulometry: radius %u: %u is not above radius %u: %u", k, radii[k], k - 1, radii[k - 1]);
            for (uint32_t k = 0; k < radius_count; k++) list.r[k] = (int)radii[k];
            list.count = (int)radius_count;
            return 1;
        },
        [&](const musica_sim_query& q, GranulometryQueryDev& d) {
            d.groups = granulometry_groups(tile_grid(d, q.w, q.h), env_int("MUSICA_GRANULOMETRY_GROUPS", 0));
            return TablePlace{d.groups, ((size_t)radius_count + 1) * 2 * kGranulometryWords};
        },
        nothing,
        [&](const GranulometryQueryDev* d_qs, int max_groups, unsigned long long* d_tables) {
            launch_sim_granulometry(c->stream, d_qs, (int)count, max_groups, list, d_tables);
        },
        nothing, [&](uint32_t i, const musica_sim_query& q, const uint64_t*) { out[i].pixels = (uint64_t)q.w * q.h; });
    ABI_CATCH("musica_sim_granulometry")
}

// ---- the contours of a comparison (musica_sim_contours, include/musica.h; kernels_contours.hip) ------------------------------------------
static_assert(kContoursMaxRadius == MUSICA_CONTOURS_MAX_RADIUS && kContoursMaxQueries == MUSICA_CONTOURS_MAX_QUERIES && kContoursMaxThreshold == MUSICA_CONTOURS_MAX_THRESHOLD,
              "kernels_contours.hip's constants are include/musica.h's");

int musica_sim_contours(musica_ctx* c, uint32_t threshold, uint32_t radius, uint32_t count, const musica_sim_query* qs, musica_sim_contours_result* out, uint64_t* tables,
                        uint64_t table_words, uint8_t* planes, uint64_t plane_bytes) {
    ABI_TRY
    size_t pixels = 0, bit_words = 0;   // of the whole call: every query's w * h, every query's two bit planes
    int max_tiles = 1;
    unsigned long long counts[kContoursMaxQueries][2] = {};
    const int ok = sim_query_tables(
        c, "musica_sim_contours", kContourBuffers, count, qs, out, tables, table_words,
        [&] {
            if (threshold < 1 || threshold > MUSICA_CONTOURS_MAX_THRESHOLD)
                return fail("musica_sim_contours: threshold %u is not in 1 .. %u", threshold, MUSICA_CONTOURS_MAX_THRESHOLD);
            if (radius < 1 || radius > MUSICA_CONTOURS_MAX_RADIUS) return fail("musica_sim_contours: radius %u is not in 1 .. %d", radius, MUSICA_CONTOURS_MAX_RADIUS);
            return 1;
        },
        [&](const musica_sim_query& q, ContourQueryDev& d) {
            const int tiles = tile_grid(d, q.w, q.h);
            max_tiles = std::max(max_tiles, tiles);
            d.groups = contours_groups(tiles, env_int("MUSICA_CONTOURS_GROUPS", 0));
            d.row_words = d.tiles_x;   // a tile column is one u64 of a bit row
            d.bits = bit_words;
            d.plane = pixels;
            bit_words += 2 * (size_t)q.h * d.row_words;
            pixels += (size_t)q.w * q.h;
            return TablePlace{d.groups, 2 * ((size_t)radius * radius + 2)};
        },
        [&] {   // behind the tables' refusals, in front of every launch and copy
            if (planes && plane_bytes < pixels)
                return fail("musica_sim_contours: plane_bytes %llu is less than the %llu bytes of the planes", (unsigned long long)plane_bytes, (unsigned long long)pixels);
            StudyState& st = c->study;
            if (!grow(c, "musica_sim_contours", &st.d_contour_bits, &st.contour_bits_cap, bit_words, "bit-plane words") ||
                (planes && !grow(c, "musica_sim_contours", &st.d_contour_planes, &st.contour_plane_cap, pixels, "plane bytes")))
                return 0;
            if (!ensure(c, &st.d_contour_counts, (size_t)kContoursMaxQueries * 2)) return fail("musica_sim_contours: device allocation failed");
            HIP_OK(hipMemsetAsync(st.d_contour_counts, 0, sizeof(counts), c->stream));
            return 1;
        },
        [&](const ContourQueryDev* d_qs, int max_groups, unsigned long long* d_tables) {
            StudyState& st = c->study;
            launch_sim_contours(c->stream, d_qs, (int)count, max_tiles, max_groups, threshold, (int)radius, st.d_contour_bits, st.d_contour_counts,
                                planes ? st.d_contour_planes : nullptr, d_tables);
        },
        [&] {
            HIP_OK(hipMemcpyAsync(counts, c->study.d_contour_counts, sizeof(counts), hipMemcpyDeviceToHost, c->stream));
            if (planes) HIP_OK(hipMemcpyAsync(planes, c->study.d_contour_planes, pixels, hipMemcpyDeviceToHost, c->stream));
            return 1;
        },
        [&](uint32_t i, const musica_sim_query& q, const uint64_t*) {
            out[i].contour_a = counts[i][0];
            out[i].contour_b = counts[i][1];
            out[i].pixels = (uint64_t)q.w * q.h;
        });
    if (!ok) return 0;
    uint64_t at = 0;   // the byte planes lie one behind the other, whether or not they were asked for
    for (uint32_t i = 0; i < count; i++) {
        out[i].plane_offset = at;
        at += out[i].pixels;
    }
    return 1;
    ABI_CATCH("musica_sim_contours")
}

// ---- the level sets of a comparison (musica_sim_minkowski, include/musica.h; kernels_minkowski.hip) --------------------------------------
static_assert(kMinkowskiMaxQueries == MUSICA_MINKOWSKI_MAX_QUERIES && kMinkowskiKinds == MUSICA_MINKOWSKI_KINDS && kMinkowskiSides == MUSICA_MINKOWSKI_SIDES,
              "kernels_minkowski.hip's constants are include/musica.h's");

int musica_sim_minkowski(musica_ctx* c, uint32_t count, const musica_sim_query* qs, musica_sim_minkowski_result* out, uint32_t* tables, uint64_t table_words) {
    ABI_TRY
    return sim_query_tables(
        c, "musica_sim_minkowski", kMinkowskiBuffers, count, qs, out, tables, table_words, nothing,
        [&](const musica_sim_query& q, MinkowskiQueryDev& d) {
            d.groups = minkowski_groups(tile_grid(d, q.w, q.h), env_int("MUSICA_MINKOWSKI_GROUPS", 0));
            return TablePlace{d.groups, (size_t)kMinkowskiSides * kMinkowskiKinds * 256};
        },
        nothing,
        [&](const MinkowskiQueryDev* d_qs, int max_groups, uint32_t* d_tables) { launch_sim_minkowski(c->stream, d_qs, (int)count, max_groups, d_tables); },
        nothing, [&](uint32_t i, const musica_sim_query& q, const uint32_t*) { out[i].pixels = (uint64_t)q.w * q.h; });
    ABI_CATCH("musica_sim_minkowski")
}

// ---- the reach of a change of the input (musica_sim_reach / musica_sim_reach_classes, include/musica.h; kernels_reach.hip) --------------
static_assert(kReachMaxRadii == MUSICA_REACH_MAX_RADII && kReachMaxRadius == MUSICA_REACH_MAX_RADIUS && kReachMaxQueries == MUSICA_REACH_MAX_QUERIES &&
                  kReachWords == MUSICA_REACH_WORDS,
              "kernels_reach.hip's limits are include/musica.h's");

// What both reach calls refuse behind their own arguments, in the same words: no source plane, a last step whose input is not a plane
// of the context's (the pair of input and output would not be coherent), and a list of radii that is not 0 < r1 < .. <= the maximum.
static int reach_check(const musica_ctx* c, const char* fn, uint32_t radii_count, const uint32_t* radii) {
    if (!c->study.d_alter_src) return fail("%s: no source plane (musica_alter_set_source)", fn);
    if (c->cur_input != c->d_input && !(c->d_input_kept && c->cur_input == c->d_input_kept) && !(c->d_input2 && c->cur_input == c->d_input2))
        return fail("%s: the last step's input is not a plane of the context's (musica_execute_device)", fn);
    if (!radii) return fail("%s: radii is NULL", fn);
    if (radii_count < 1 || radii_count > MUSICA_REACH_MAX_RADII) return fail("%s: radii_count %u out of range [1, %d]", fn, radii_count, MUSICA_REACH_MAX_RADII);
    if (radii[0] != 0) return fail("%s: radii[0] is %u, not 0", fn, radii[0]);
    for (uint32_t k = 0; k < radii_count; k++) {
        if (k && radii[k] <= radii[k - 1]) return fail("%s: radii[%u] = %u does not ascend from radii[%u] = %u", fn, k, radii[k], k - 1, radii[k - 1]);
        if (radii[k] > MUSICA_REACH_MAX_RADIUS) return fail("%s: radii[%u] = %u is above %d", fn, k, radii[k], MUSICA_REACH_MAX_RADIUS);
    }
    return 1;
}

// The radii on the device and the summed-area table of source != the input of image idx's current output, enqueued on the stream.
static int reach_table(musica_ctx* c, const char* fn, uint32_t idx, uint32_t radii_count, const uint32_t* radii) {
    StudyState& st = c->study;
    if (!ensure(c, &st.d_reach_radii, MUSICA_REACH_MAX_RADII)) return fail("%s: device allocation failed", fn);
    if (!scatter_plane(c, fn)) return 0;
    HIP_OK(hipMemcpyAsync(st.d_reach_radii, radii, radii_count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    launch_reach_table(c->stream, st.d_alter_src, c->cur_input + idx * (size_t)c->N * c->N, st.d_scatter, c->N);
    HIP_OK(hipGetLastError());
    return 1;
}

int musica_sim_reach(musica_ctx* c, uint32_t radii_count, const uint32_t* radii, uint32_t count, const musica_sim_query* qs, musica_sim_reach_result* out,
                     uint64_t* tables, uint64_t table_words) {
    ABI_TRY
    const size_t classes = (size_t)radii_count + 1;
    uint32_t seeds = 0;
    return sim_query_tables(
        c, "musica_sim_reach", kReachBuffers, count, qs, out, tables, table_words,
        [&] {
            if (!reach_check(c, "musica_sim_reach", radii_count, radii)) return 0;
            for (uint32_t i = 1; i < count; i++)
                if (qs[i].image_index != qs[0].image_index)
                    return fail("musica_sim_reach: query %u names image %u, query 0 image %u: one call, one input plane", i, qs[i].image_index, qs[0].image_index);
            return 1;
        },
        [&](const musica_sim_query& q, ReachQueryDev& d) {
            d.sx = (int)q.ax + MUSICA_OUT_MARGIN;   // the class is taken at side a's coordinates
            d.sy = (int)q.ay + MUSICA_OUT_MARGIN;
            return TablePlace{tile_grid(d, q.w, q.h), classes * kReachWords};
        },
        [&] { return reach_table(c, "musica_sim_reach", qs[0].image_index, radii_count, radii); },
        [&](const ReachQueryDev* d_qs, int max_tiles, unsigned long long* d_tables) {
            launch_sim_reach(c->stream, d_qs, (int)count, max_tiles, c->study.d_scatter, c->N, c->study.d_reach_radii, (int)radii_count, d_tables);
        },
        [&] {   // the summed-area table's last entry
            HIP_OK(hipMemcpyAsync(&seeds, c->study.d_scatter + (size_t)c->N * c->N - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            return 1;
        },
        [&](uint32_t i, const musica_sim_query& q, const uint64_t* t) {
            out[i].classes = classes;
            out[i].ssd = column_sum(t, classes, kReachWords, 4);
            out[i].pixels = (uint64_t)q.w * q.h;
            out[i].seeds = seeds;
        });
    ABI_CATCH("musica_sim_reach")
}

int musica_sim_reach_classes(musica_ctx* c, uint32_t idx, uint32_t radii_count, const uint32_t* radii, uint8_t* dst) {
    ABI_TRY
    if (!c) return fail("musica_sim_reach_classes: ctx is NULL");
    if (!dst) return fail("musica_sim_reach_classes: dst is NULL");
    if (c->N <= 2 * MUSICA_OUT_MARGIN) return fail("musica_sim_reach_classes: image too small for the %d-pixel margin", MUSICA_OUT_MARGIN);
    if (!check_img(c, "musica_sim_reach_classes", idx)) return 0;
    if (!reach_check(c, "musica_sim_reach_classes", radii_count, radii)) return 0;
    CHECK_CTX(c);
    StudyState& st = c->study;
    const size_t px = sim_side(c) * sim_side(c);
    if (!ensure(c, &st.d_reach_classes, px)) return fail("musica_sim_reach_classes: device allocation failed");
    if (!reach_table(c, "musica_sim_reach_classes", idx, radii_count, radii)) return 0;
    launch_reach_classes(c->stream, st.d_scatter, c->N, MUSICA_OUT_MARGIN, st.d_reach_radii, (int)radii_count, st.d_reach_classes);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(dst, st.d_reach_classes, px, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));   // radii and dst are the caller's again
    return 1;
    ABI_CATCH("musica_sim_reach_classes")
}

// ---- ensemble statistics (musica_sim_ensemble_*, include/musica.h; kernels_ensemble.hip) ------------------------------------------------
int musica_sim_ensemble_reset(musica_ctx* c) {
    ABI_TRY
    if (!c) return fail("musica_sim_ensemble_reset: ctx is NULL");
    if (c->N <= 2 * MUSICA_OUT_MARGIN) return fail("musica_sim_ensemble_reset: image too small for the %d-pixel margin", MUSICA_OUT_MARGIN);
    CHECK_CTX(c);
    StudyState& st = c->study;
    const size_t px = sim_side(c) * sim_side(c);
    if (!ensure(c, &st.d_ens, px)) return fail("musica_sim_ensemble_reset: device allocation of %zu bytes failed", px * sizeof(uint2));
    HIP_OK(hipMemsetAsync(st.d_ens, 0, px * sizeof(uint2), c->stream));   // behind the adds and results the stream holds
    st.ens_k = 0;
    st.ens_reset = true;
    st.cov_regions = 0;   // tracking ends with the ensemble it was declared for
    return 1;
    ABI_CATCH("musica_sim_ensemble_reset")
}

int musica_sim_ensemble_add(musica_ctx* c, uint32_t first, uint32_t count) {
    ABI_TRY
    if (!c) return fail("musica_sim_ensemble_add: ctx is NULL");
    if (count == 0) return fail("musica_sim_ensemble_add: count is 0");
    if ((uint64_t)first + count > (uint64_t)c->B) return fail("musica_sim_ensemble_add: images %u .. %u + %u exceed the batch of %d", first, first, count, c->B);
    if (c->N <= 2 * MUSICA_OUT_MARGIN) return fail("musica_sim_ensemble_add: image too small for the %d-pixel margin", MUSICA_OUT_MARGIN);
    if (!c->stepped) return fail("musica_sim_ensemble_add: no step has run on this context");
    StudyState& st = c->study;
    if (!st.ens_reset) return fail("musica_sim_ensemble_add: the ensemble was never reset (musica_sim_ensemble_reset)");
    if ((uint64_t)st.ens_k + count > MUSICA_SIM_ENSEMBLE_MAX)
        return fail("musica_sim_ensemble_add: %u + %u realisations exceed MUSICA_SIM_ENSEMBLE_MAX = %d", st.ens_k, count, MUSICA_SIM_ENSEMBLE_MAX);
    CHECK_CTX(c);
    launch_ens_add(c->stream, image_slice(c, c->d_graded, first), c->lv[0], (int)count, st.d_ens);
    if (st.cov_regions)   // musica_sim_ensemble_track: the same images' lag products, behind the accumulation
        launch_cov_add(c->stream, st.d_cov_r, (int)st.cov_regions, st.cov_max_tiles, (int)st.cov_radius, image_slice(c, c->d_graded, first), c->lv[0],
                       (int)count, st.d_cov_tiles);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("musica_sim_ensemble_add: launch failed: %s", hipGetErrorString(e));
    st.ens_k += count;
    return 1;
    ABI_CATCH("musica_sim_ensemble_add")
}

int musica_sim_ensemble_get(musica_ctx* c, uint32_t* s1, uint32_t* s2, uint32_t* realisations) {
    ABI_TRY
    if (!c) return fail("musica_sim_ensemble_get: ctx is NULL");
    StudyState& st = c->study;
    if (!st.ens_reset) return fail("musica_sim_ensemble_get: the ensemble was never reset (musica_sim_ensemble_reset)");
    CHECK_CTX(c);
    const size_t px = sim_side(c) * sim_side(c);
    std::vector<uint2> words(s1 || s2 ? px : 0);
    if (!words.empty()) HIP_OK(hipMemcpyAsync(words.data(), st.d_ens, px * sizeof(uint2), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < words.size(); i++) {
        if (s1) s1[i] = words[i].x;
        if (s2) s2[i] = words[i].y;
    }
    if (realisations) *realisations = st.ens_k;
    return 1;
    ABI_CATCH("musica_sim_ensemble_get")
}

// musica_sim_ensemble_result's doubles from the exact integers, one operation each in the order include/musica.h states
// (harness.ensemble_summary restates them).
static void ensemble_finish(const unsigned long long* r /* kEnsTotals */, uint32_t K, const musica_sim_query& q, musica_sim_ensemble_stats* o) {
    const uint64_t n = (uint64_t)q.w * q.h, k = K;
    memset(o, 0, sizeof(*o));
    o->sq_bias_sum = r[0];
    o->var_sum = r[1];
    o->bias_sum = (int64_t)r[2];
    o->sq_err_sum = r[3];
    o->abs_bias_max = r[4];
    o->var_max = r[5];
    o->pixels = n;
    o->realisations = K;
    o->tiles_x = (uint32_t)tiles_along(q.w);
    o->tiles_y = (uint32_t)tiles_along(q.h);
    o->mean_shift = (double)o->bias_sum / (double)(k * n);
    o->bias_rms = sqrt((double)o->sq_bias_sum / (double)(k * k * n));
    o->noise_rms = K == 1 ? 0.0 : sqrt((double)o->var_sum / (double)(k * (k - 1) * n));
    o->mse = 1.0 - sqrt((double)o->sq_err_sum / (double)(k * n)) / 255.0;
    const uint64_t both = o->sq_bias_sum + o->var_sum;   // == K sq_err_sum < 2^64
    o->bias_fraction = both == 0 ? 0.0 : (double)o->sq_bias_sum / (double)both;
}

int musica_sim_ensemble_result(musica_ctx* c, uint32_t count, const musica_sim_query* qs, musica_sim_ensemble_stats* out, uint64_t* tile_tables) {
    ABI_TRY
    if (!sim_check_queries(c, "musica_sim_ensemble_result", count, qs, out)) return 0;
    StudyState& st = c->study;
    if (!st.ens_reset || st.ens_k == 0) return fail("musica_sim_ensemble_result: the ensemble holds no realisation (musica_sim_ensemble_reset, _add)");
    const uint32_t K = st.ens_k;
    for (uint32_t i = 0; i < count; i++)   // sum D^2 <= 255^2 K^2 w h must fit u64; every other sum is smaller
        if (((unsigned __int128)65025u * K * K * qs[i].w * qs[i].h) >> 64)
            return fail("musica_sim_ensemble_result: query %u: 65025 * %u^2 * %u * %u does not fit 64 bits", i, K, qs[i].w, qs[i].h);
    const size_t nw = sim_side(c);
    std::vector<EnsQueryDev> hq(count);
    TileRun run;
    for (uint32_t i = 0; i < count; i++) {
        const musica_sim_query& q = qs[i];
        EnsQueryDev& d = hq[i];
        d.s = st.d_ens + (size_t)q.ay * nw + q.ax;
        d.b = st.slot[q.slot] + (size_t)q.by * nw + q.bx;
        d.s_pitch = d.b_pitch = (int)nw;
        d.w = (int)q.w;
        d.h = (int)q.h;
        run.place(d, 1);
    }
    const size_t tiles = run.next;
    CHECK_CTX(c);
    if (!(ensure(c, &st.d_ens_q, MUSICA_SIM_MAX_QUERIES) && ensure(c, &st.d_ens_out, (size_t)MUSICA_SIM_MAX_QUERIES * kEnsTotals)))
        return fail("musica_sim_ensemble_result: device allocation failed");
    if (!grow(c, "musica_sim_ensemble_result", &st.d_ens_tiles, &st.ens_tiles_cap, tiles, "tile pairs", 2)) return 0;
    HIP_OK(hipMemcpyAsync(st.d_ens_q, hq.data(), count * sizeof(EnsQueryDev), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemsetAsync(st.d_ens_out, 0, (size_t)count * kEnsTotals * sizeof(unsigned long long), c->stream));
    launch_ens_stats(c->stream, st.d_ens_q, (int)count, run.max_tiles, K, st.d_ens_tiles, st.d_ens_out);
    HIP_OK(hipGetLastError());
    std::vector<unsigned long long> res((size_t)count * kEnsTotals);
    HIP_OK(hipMemcpyAsync(res.data(), st.d_ens_out, res.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if (tile_tables) HIP_OK(hipMemcpyAsync(tile_tables, st.d_ens_tiles, 2 * tiles * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));   // hq and the results are read by then
    for (uint32_t i = 0; i < count; i++) ensemble_finish(res.data() + (size_t)i * kEnsTotals, K, qs[i], out + i);
    return 1;
    ABI_CATCH("musica_sim_ensemble_result")
}

// ---- the noise's spatial covariance (musica_sim_ensemble_track / _covariance, include/musica.h; kernels_covariance.hip) ---------------
int musica_sim_ensemble_track(musica_ctx* c, uint32_t radius, uint32_t count, const musica_sim_query* qs) {
    ABI_TRY
    if (!c) return fail("musica_sim_ensemble_track: ctx is NULL");
    if (!qs) return fail("musica_sim_ensemble_track: regions is NULL");
    if (radius < 1 || radius > MUSICA_SIM_MAX_RADIUS) return fail("musica_sim_ensemble_track: radius %u out of range [1, %d]", radius, MUSICA_SIM_MAX_RADIUS);
    if (count == 0 || count > MUSICA_SIM_COV_MAX_REGIONS) return fail("musica_sim_ensemble_track: count %u out of range [1, %d]", count, MUSICA_SIM_COV_MAX_REGIONS);
    StudyState& st = c->study;
    if (!st.ens_reset) return fail("musica_sim_ensemble_track: the ensemble was never reset (musica_sim_ensemble_reset)");
    if (st.ens_k) return fail("musica_sim_ensemble_track: %u realisations were already added: track after the reset, before the first add", st.ens_k);
    if (!sim_check_queries(c, "musica_sim_ensemble_track", count, qs, qs)) return 0;
    const uint64_t nw = sim_side(c);
    const size_t T = (size_t)(radius + 1) * (2 * radius + 1);
    std::vector<CovRegionDev> hr(count);
    TileRun run;
    for (uint32_t i = 0; i < count; i++) {
        const musica_sim_query& q = qs[i];
        if (q.ax < radius || (uint64_t)q.ax + q.w + radius > nw || (uint64_t)q.ay + q.h + radius > nw)
            return fail("musica_sim_ensemble_track: region %u: the window (%u, %u) + %u x %u grown by the radius %u (left, right, down) leaves the %llu x %llu plane",
                        i, q.ax, q.ay, q.w, q.h, radius, (unsigned long long)nw, (unsigned long long)nw);
        if (((unsigned __int128)65025u * MUSICA_SIM_ENSEMBLE_MAX * MUSICA_SIM_ENSEMBLE_MAX * q.w * q.h) >> 63)
            return fail("musica_sim_ensemble_track: region %u: 65025 * %d^2 * %u * %u does not fit 63 bits", i, MUSICA_SIM_ENSEMBLE_MAX, q.w, q.h);
        CovRegionDev& d = hr[i];
        d.ax = (int)q.ax;
        d.ay = (int)q.ay;
        d.w = (int)q.w;
        d.h = (int)q.h;
        run.place(d, T);
    }
    const size_t words = run.next;
    CHECK_CTX(c);
    if (!(ensure(c, &st.d_cov_r, MUSICA_SIM_COV_MAX_REGIONS) &&
          ensure(c, &st.d_cov_tables, (size_t)MUSICA_SIM_COV_MAX_REGIONS * (MUSICA_SIM_MAX_RADIUS + 1) * (2 * MUSICA_SIM_MAX_RADIUS + 1))))
        return fail("musica_sim_ensemble_track: device allocation failed");
    if (!grow(c, "musica_sim_ensemble_track", &st.d_cov_tiles, &st.cov_tiles_cap, words, "tile-table words", 1, &st.d_cov_ctiles)) return 0;
    HIP_OK(hipMemsetAsync(st.d_cov_tiles, 0, words * sizeof(unsigned long long), c->stream));   // behind what the stream holds
    HIP_OK(hipMemcpyAsync(st.d_cov_r, hr.data(), count * sizeof(CovRegionDev), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));   // hr is read by then
    for (uint32_t i = 0; i < count; i++) st.cov_q[i] = qs[i];
    st.cov_radius = radius;
    st.cov_max_tiles = run.max_tiles;
    st.cov_words = words;
    st.cov_regions = count;
    return 1;
    ABI_CATCH("musica_sim_ensemble_track")
}

// musica_sim_ensemble_covariance's doubles from one exact table, one operation each in the order include/musica.h states
// (harness.covariance_summary restates them).
static void covariance_finish(const int64_t* Ct, uint32_t K, uint32_t radius, const musica_sim_query& q, musica_sim_cov_result* o) {
    const uint64_t n = (uint64_t)q.w * q.h, k = K;
    const int R = (int)radius, S = 2 * R + 1;
    memset(o, 0, sizeof(*o));
    const int64_t c00 = Ct[R];
    o->c00 = c00;
    o->pixels = n;
    o->realisations = K;
    o->radius = radius;
    o->tiles_x = (uint32_t)tiles_along(q.w);
    o->tiles_y = (uint32_t)tiles_along(q.h);
    o->noise_var = K == 1 ? 0.0 : (double)c00 / (double)(k * (k - 1) * n);
    o->rho_x = c00 == 0 ? 0.0 : (double)Ct[R + 1] / (double)c00;
    o->rho_y = c00 == 0 ? 0.0 : (double)Ct[S + R] / (double)c00;
    double half = 0.0;
    for (int dy = 0; dy <= R; dy++)
        for (int dx = dy ? -R : 1; dx <= R; dx++) half += (double)Ct[dy * S + dx + R];
    o->corr_area = c00 == 0 ? 1.0 : ((double)c00 + 2.0 * half) / (double)c00;
}

int musica_sim_ensemble_covariance(musica_ctx* c, musica_sim_cov_result* out, int64_t* tables, int64_t* tile_tables) {
    ABI_TRY
    if (!c) return fail("musica_sim_ensemble_covariance: ctx is NULL");
    if (!out) return fail("musica_sim_ensemble_covariance: results is NULL");
    StudyState& st = c->study;
    if (!st.ens_reset || !st.cov_regions) return fail("musica_sim_ensemble_covariance: no region is tracked (musica_sim_ensemble_track)");
    if (st.ens_k == 0) return fail("musica_sim_ensemble_covariance: the ensemble holds no realisation (musica_sim_ensemble_add)");
    const uint32_t K = st.ens_k, count = st.cov_regions, radius = st.cov_radius;
    const size_t T = (size_t)(radius + 1) * (2 * radius + 1);
    CHECK_CTX(c);
    HIP_OK(hipMemsetAsync(st.d_cov_tables, 0, count * T * sizeof(unsigned long long), c->stream));
    launch_cov_mean(c->stream, st.d_cov_r, (int)count, st.cov_max_tiles, (int)radius, K, st.d_ens, (int)sim_side(c), st.d_cov_tiles, st.d_cov_ctiles,
                    st.d_cov_tables);
    HIP_OK(hipGetLastError());
    std::vector<int64_t> own;
    if (!tables) {
        own.resize(count * T);
        tables = own.data();
    }
    HIP_OK(hipMemcpyAsync(tables, st.d_cov_tables, count * T * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (tile_tables) HIP_OK(hipMemcpyAsync(tile_tables, st.d_cov_ctiles, st.cov_words * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < count; i++) covariance_finish(tables + (size_t)i * T, K, radius, st.cov_q[i], out + i);
    return 1;
    ABI_CATCH("musica_sim_ensemble_covariance")
}

// ---- alterations of the study (musica_alter_*, include/musica.h; kernels_alteration.hip) ----------------------------------------------
int musica_alter_set_source(musica_ctx* c, const uint16_t* pixels) {
    if (!c) return fail("musica_alter_set_source: ctx is NULL");
    if (!pixels) return fail("musica_alter_set_source: pixels is NULL");
    CHECK_CTX(c);
    const size_t nn = (size_t)c->N * c->N;
    if (!ensure(c, &c->study.d_alter_src, nn)) return fail("musica_alter_set_source: device allocation failed");
    HIP_OK(hipMemcpyAsync(c->study.d_alter_src, pixels, nn * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));   // after alterations that read it
    HIP_OK(hipStreamSynchronize(c->stream));
    return 1;
}

static bool alter_scratch(musica_ctx* c) { return ensure(c, &c->study.d_alter_hist, 768) && ensure(c, &c->study.d_alter_fill, 1); }

// The region's percentile into d_alter_fill, on the stream.
static int enqueue_percentile(musica_ctx* c, int x, int y, int w, int h, double q) {
    PctRegion g{c->study.d_alter_src, c->N, x, y, w, h, q};
    HIP_OK(hipMemsetAsync(c->study.d_alter_hist, 0, 768 * sizeof(uint32_t), c->stream));
    launch_percentile(c->stream, g, c->study.d_alter_hist, c->study.d_alter_fill);
    HIP_OK(hipGetLastError());
    return 1;
}

// Checks `s` and restates its geometry (harness.clamp_translation / clamp_rotate / apply_collimator) as the kernel's arguments. No device work.
static int alter_args(musica_ctx* c, const char* fn, const musica_alteration* s, AlterDev& a) {
    if (!s) return fail("%s: spec is NULL", fn);
    if (!c->study.d_alter_src) return fail("%s: no source plane (musica_alter_set_source)", fn);
    if (s->kind >= MUSICA_ALTER_KIND_COUNT) return fail("%s: kind %u out of range", fn, s->kind);
    const int n = c->N;
    a = AlterDev{};
    a.kind = (int)s->kind;
    a.n = n;
    a.key0 = (uint32_t)s->seed;
    a.key1 = (uint32_t)(s->seed >> 32);
    a.stream = s->stream;
    switch (s->kind) {
        case MUSICA_ALTER_TRANSLATE: {
            const int dx = s->dx, dy = s->dy;
            if (dx >= n || dx <= -n || dy >= n || dy <= -n) return fail("%s: shift (%d, %d) leaves nothing of a %d-pixel image", fn, dx, dy, n);
            const int margin = 10;   // clamp_translation's bright = 2, margin = 10
            a.left = dx > 0 ? margin : 0;
            a.top = dy > 0 ? margin : 0;
            const int right = dx < 0 ? n - margin : n, bottom = dy < 0 ? n - margin : n;
            a.xs = std::max(dx, 0);
            a.ys = std::max(dy, 0);
            a.ww = std::min(right - a.left, n - a.xs);
            a.hh = std::min(bottom - a.top, n - a.ys);
            break;
        }
        case MUSICA_ALTER_ROTATE:
            if (s->margin < 0 || 2 * (int64_t)s->margin >= n) return fail("%s: margin %d leaves no crop of a %d-pixel image", fn, s->margin, n);
            if (!finite_all(s->matrix, 4) || !finite_all(s->offset, 2)) return fail("%s: matrix or offset is not finite", fn);
            a.margin = s->margin;
            a.crop = n - 2 * s->margin;
            memcpy(a.m, s->matrix, sizeof(a.m));
            memcpy(a.off, s->offset, sizeof(a.off));
            break;
        case MUSICA_ALTER_COLLIMATOR:
            if (s->shutter_h < 0 || s->shutter_v < 0 || 2 * (int64_t)s->shutter_h > n || 2 * (int64_t)s->shutter_v > n)
                return fail("%s: shutters (%d, %d) leave nothing of a %d-pixel image", fn, s->shutter_h, s->shutter_v, n);
            a.sh = s->shutter_h;
            a.sv = s->shutter_v;
            break;
        case MUSICA_ALTER_GAUSSIAN:
            if (!std::isfinite(s->mean) || !std::isfinite(s->sigma) || !(s->sigma > 0.0)) return fail("%s: mean %g / sigma %g: need finite values, sigma > 0", fn, s->mean, s->sigma);
            a.mean = s->mean;
            a.sigma = s->sigma;
            break;
        case MUSICA_ALTER_POISSON:
            if (!std::isfinite(s->factor) || !(s->factor > 0.0) || 65535.0 * s->factor >= 1073741824.0)
                return fail("%s: factor %g: need a finite factor > 0 with 65535 * factor < 2^30", fn, s->factor);
            a.factor = s->factor;
            break;
        case MUSICA_ALTER_SYMMETRY:
            if (s->dx < 0 || s->dx > 7) return fail("%s: element %d is not one of the square's 8 symmetries (0 .. 7)", fn, s->dx);
            break;
        default: break;
    }
    return 1;
}

int musica_alter(musica_ctx* c, uint32_t idx, const musica_alteration* s) {
    if (!c) return fail("musica_alter: ctx is NULL");
    AlterDev a;
    if (!alter_args(c, "musica_alter", s, a)) return 0;
    CHECK_IMG(c, idx);
    CHECK_CTX(c);
    if (!alter_scratch(c)) return fail("musica_alter: device allocation failed");
    const size_t nn = (size_t)c->N * c->N;
    if (!alter_keep_input(c, "musica_alter")) return 0;
    const double* fill = nullptr;
    if (s->kind == MUSICA_ALTER_TRANSLATE) {   // clamp_translation: the 99th percentile of image[top:b_bottom, left:b_right]
        const int n = c->N, b_right = s->dx > 0 ? 12 : n, b_bottom = s->dy > 0 ? 12 : n;
        if (!enqueue_percentile(c, a.left, a.top, b_right - a.left, b_bottom - a.top, 99.0)) return 0;
        fill = c->study.d_alter_fill;
    } else if (s->kind == MUSICA_ALTER_ROTATE) {   // clamp_rotate: the 95th percentile of the crop
        if (!enqueue_percentile(c, a.margin, a.margin, a.crop, a.crop, 95.0)) return 0;
        fill = c->study.d_alter_fill;
    }
    if (s->kind == MUSICA_ALTER_SYMMETRY) launch_symmetry_u16(c->stream, c->study.d_alter_src, c->d_input + idx * nn, c->N, s->dx);   // a permutation: kernels_symmetry.hip
    else launch_alter(c->stream, c->study.d_alter_src, c->d_input + idx * nn, nullptr, a, fill);
    HIP_OK(hipGetLastError());
    return 1;
}

int musica_alter_blur(musica_ctx* c, uint32_t idx, uint32_t radius) {
    return alter_into(
        c, "musica_alter_blur", nullptr, idx,
        [&] { return radius < 1 || radius > MUSICA_BLUR_MAX_RADIUS ? fail("musica_alter_blur: radius %u out of range [1, %d]", radius, MUSICA_BLUR_MAX_RADIUS) : 1; },
        nothing, [&](const uint16_t* src, uint16_t* dst) { launch_blur_u16(c->stream, src, dst, c->N, (int)radius); });   // kernels_blur.hip
}

int musica_alter_codec(musica_ctx* c, uint32_t idx, const uint16_t table[64]) {
    CodecTable t;
    return alter_into(
        c, "musica_alter_codec", table ? nullptr : "table", idx, [&] { return codec_check("musica_alter_codec", table, 0, t); }, nothing,
        [&](const uint16_t* src, uint16_t* dst) { launch_codec_u16(c->stream, src, dst, c->N, 0, t); });   // kernels_codec.hip
}

int musica_alter_zoom(musica_ctx* c, uint32_t idx, uint32_t p, uint32_t q) {
    return alter_into(c, "musica_alter_zoom", nullptr, idx, [&] { return zoom_check("musica_alter_zoom", p, q); }, nothing,
                      [&](const uint16_t* src, uint16_t* dst) { launch_zoom_u16(c->stream, src, dst, c->N, (int)p, (int)q); });   // kernels_zoom.hip
}

int musica_alter_scatter(musica_ctx* c, uint32_t idx, uint32_t radius, uint32_t num, uint32_t den) {
    return alter_into(c, "musica_alter_scatter", nullptr, idx, [&] { return scatter_check("musica_alter_scatter", radius, num, den); },
                      [&] { return scatter_plane(c, "musica_alter_scatter"); }, [&](const uint16_t* src, uint16_t* dst) {
                          launch_scatter_u16(c->stream, src, dst, c->study.d_scatter, c->N, (int)radius, (int)num, (int)den);   // kernels_scatter.hip
                      });
}

int musica_alter_warp(musica_ctx* c, uint32_t idx, const int16_t* field, uint32_t nodes) {
    ABI_TRY
    std::vector<uint32_t> packed;
    int m = 0;
    return alter_into(
        c, "musica_alter_warp", !field ? "field" : nullptr, idx, [&] { return warp_check("musica_alter_warp", field, nodes, 0, (size_t)c->N, packed, &m); },
        [&] { return warp_upload(c, "musica_alter_warp", packed); },
        [&](const uint16_t* src, uint16_t* dst) { launch_warp_u16(c->stream, src, dst, c->N, c->study.d_warp_nodes, m, 0); });   // kernels_warp.hip
    ABI_CATCH("musica_alter_warp")
}

int musica_alter_details(musica_ctx* c, uint32_t idx, uint32_t count, const musica_detail* details) {
    ABI_TRY
    std::vector<PackedDetail> packed;
    return alter_into(
        c, "musica_alter_details", !details ? "details" : nullptr, idx, [&] { return details_check("musica_alter_details", count, details, c->N, true, packed); },
        [&] { return upload_list(c, "musica_alter_details", kDetailBuffers, packed); },
        [&](const uint16_t* src, uint16_t* dst) { launch_alter_details(c->stream, src, dst, c->N, c->study.d_details, (int)count); });   // kernels_details.hip
    ABI_CATCH("musica_alter_details")
}

int musica_alter_edges(musica_ctx* c, uint32_t idx, uint32_t count, const musica_edge* edges) {
    ABI_TRY
    std::vector<PackedEdge> packed;
    uint64_t words = 0;
    return alter_into(
        c, "musica_alter_edges", !edges ? "edges" : nullptr, idx, [&] { return edges_check("musica_alter_edges", count, edges, c->N, true, packed, &words); },
        [&] { return upload_list(c, "musica_alter_edges", kEdgeBuffers, packed); },
        [&](const uint16_t* src, uint16_t* dst) { launch_alter_edges(c->stream, src, dst, c->N, c->study.d_edges, (int)count); });   // kernels_edges.hip
    ABI_CATCH("musica_alter_edges")
}

int musica_alter_gratings(musica_ctx* c, uint32_t idx, uint32_t count, const musica_grating* gratings, const int16_t* waves, uint64_t wave_words) {
    ABI_TRY
    std::vector<PackedGrating> packed;
    uint64_t periods = 0;
    return alter_into(
        c, "musica_alter_gratings", !gratings || !waves ? "gratings or waves" : nullptr, idx,
        [&] {
            if (!gratings_check("musica_alter_gratings", count, gratings, c->N, packed, &periods)) return 0;
            if (wave_words < periods)
                return fail("musica_alter_gratings: wave_words %llu is less than the %llu entries of the waves", (unsigned long long)wave_words, (unsigned long long)periods);
            for (uint64_t i = 0; i < periods; i++)
                if (waves[i] < -MUSICA_GRATING_MAX_CONTRAST || waves[i] > MUSICA_GRATING_MAX_CONTRAST)
                    return fail("musica_alter_gratings: wave entry %llu is %d, beyond +-%d", (unsigned long long)i, (int)waves[i], MUSICA_GRATING_MAX_CONTRAST);
            return 1;
        },
        [&] {
            if (!ensure(c, &c->study.d_grating_waves, (size_t)MUSICA_GRATING_MAX * MUSICA_GRATING_MAX_PERIOD))
                return fail("musica_alter_gratings: device allocation of the waves failed");
            HIP_OK(hipMemcpyAsync(c->study.d_grating_waves, waves, (size_t)periods * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
            return upload_list(c, "musica_alter_gratings", kGratingBuffers, packed);   // synchronises: the caller's waves have been read
        },
        [&](const uint16_t* src, uint16_t* dst) {
            launch_alter_gratings(c->stream, src, dst, c->N, c->study.d_gratings, c->study.d_grating_waves, (int)count);   // kernels_gratings.hip
        });
    ABI_CATCH("musica_alter_gratings")
}

int musica_alter_points(musica_ctx* c, uint32_t idx, uint32_t count, const musica_defect* points) {
    ABI_TRY
    std::vector<PackedPoint> packed;
    return alter_into(
        c, "musica_alter_points", !points ? "points" : nullptr, idx,
        [&] { return points_check("musica_alter_points", count, points, c->N, true, MUSICA_POINT_MAX_GROUPS, packed); },
        [&] {
            point_rows(packed, c->N);   // ordered by y, each tile row's range behind the points
            return upload_list(c, "musica_alter_points", kPointBuffers, packed);
        },
        [&](const uint16_t* src, uint16_t* dst) { launch_alter_points(c->stream, src, dst, c->N, c->study.d_points, (int)count); });   // kernels_points.hip
    ABI_CATCH("musica_alter_points")
}

int musica_alter_gain(musica_ctx* c, uint32_t idx, const uint16_t* gx, const uint16_t* gy) {
    ABI_TRY
    return alter_into(
        c, "musica_alter_gain", !gx || !gy ? "gx or gy" : nullptr, idx, nothing,
        [&] {
            if (!(ensure(c, &c->study.d_gain_x, (size_t)c->N) && ensure(c, &c->study.d_gain_y, (size_t)c->N)))
                return fail("musica_alter_gain: device allocation of the tables failed");
            const std::vector<uint32_t> wide(gy, gy + c->N);   // the kernel fetches a row's gain on the scalar side: u32
            HIP_OK(hipMemcpyAsync(c->study.d_gain_x, gx, (size_t)c->N * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
            HIP_OK(hipMemcpyAsync(c->study.d_gain_y, wide.data(), (size_t)c->N * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            HIP_OK(hipStreamSynchronize(c->stream));   // the caller's tables and `wide` have been read
            return 1;
        },
        [&](const uint16_t* src, uint16_t* dst) { launch_alter_gain(c->stream, src, dst, c->N, c->study.d_gain_x, c->study.d_gain_y); });   // kernels_gain.hip
    ABI_CATCH("musica_alter_gain")
}

int musica_alter_lut(musica_ctx* c, uint32_t idx, const uint16_t* lut) {
    ABI_TRY
    return alter_into(
        c, "musica_alter_lut", !lut ? "lut" : nullptr, idx, nothing,
        [&] {
            if (!ensure(c, &c->study.d_lut, (size_t)MUSICA_LUT_ENTRIES)) return fail("musica_alter_lut: device allocation of the table failed");
            HIP_OK(hipMemcpyAsync(c->study.d_lut, lut, (size_t)MUSICA_LUT_ENTRIES * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
            HIP_OK(hipStreamSynchronize(c->stream));   // the caller's table has been read
            return 1;
        },
        [&](const uint16_t* src, uint16_t* dst) { launch_alter_lut(c->stream, src, dst, c->N, c->study.d_lut); });   // kernels_levels.hip
    ABI_CATCH("musica_alter_lut")
}

int musica_alter_draws(musica_ctx* c, const musica_alteration* s, int32_t* dst) {
    ABI_TRY
    if (!c) return fail("musica_alter_draws: ctx is NULL");
    if (!dst) return fail("musica_alter_draws: dst is NULL");
    AlterDev a;
    if (!alter_args(c, "musica_alter_draws", s, a)) return 0;
    if (s->kind != MUSICA_ALTER_COLLIMATOR && s->kind != MUSICA_ALTER_GAUSSIAN && s->kind != MUSICA_ALTER_POISSON)
        return fail("musica_alter_draws: kind %u draws no noise", s->kind);
    CHECK_CTX(c);
    const size_t nn = (size_t)c->N * c->N;
    if (!ensure(c, &c->study.d_alter_draws, nn)) return fail("musica_alter_draws: device allocation failed");
    launch_alter(c->stream, c->study.d_alter_src, nullptr, c->study.d_alter_draws, a, nullptr);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(dst, c->study.d_alter_draws, nn * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 1;
    ABI_CATCH("musica_alter_draws")
}

int musica_alter_percentile(musica_ctx* c, uint32_t x, uint32_t y, uint32_t w, uint32_t h, double q, double* out) {
    if (!c) return fail("musica_alter_percentile: ctx is NULL");
    if (!out) return fail("musica_alter_percentile: out is NULL");
    if (!c->study.d_alter_src) return fail("musica_alter_percentile: no source plane (musica_alter_set_source)");
    if (w == 0 || h == 0 || (uint64_t)x + w > (uint64_t)c->N || (uint64_t)y + h > (uint64_t)c->N)
        return fail("musica_alter_percentile: region (%u, %u) + %u x %u is empty or leaves the %d-pixel plane", x, y, w, h, c->N);
    if (!(q >= 0.0 && q <= 100.0)) return fail("musica_alter_percentile: q %g outside [0, 100]", q);
    CHECK_CTX(c);
    if (!alter_scratch(c)) return fail("musica_alter_percentile: device allocation failed");
    if (!enqueue_percentile(c, (int)x, (int)y, (int)w, (int)h, q)) return 0;
    HIP_OK(hipMemcpyAsync(out, c->study.d_alter_fill, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 1;
}

}  // extern "C"
