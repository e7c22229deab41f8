// pyramid_march.h — the device code of the streaming Laplacian-pyramid marches for gfx950 (CDNA4), shared by the two translation
// units that launch them (kernels_pyramid.hip and kernels_expand_sd.hip):
//
//   reduce_band_block : img_smooth.comp + img_downsample.comp and img_upsample.comp + img_smooth_upsampled.comp +
//                       img_difference.comp in one march                    (K5 + K6 and K7 + K8 + K9; level 0: K1 + K4 on the way)
//   expand_march      : contrast_curve_apply.comp + noise_reduction.comp + img_upsample.comp +
//                       img_smooth_upsampled.comp + img_addition.comp fused (K14 + K16 + K7 + K8 + K17), the body of k_expand_fast
//
// Streaming ("fast") form, used when the level side S is a multiple of 8: one 64-lane wavefront
// owns a strip of 512 fine columns (8 per lane, two 16-byte loads per row) and marches down a
// segment of rows keeping the row window in registers; the vertical 5-tap pass runs straight
// from the loaded registers, the horizontal pass takes its 2+1 neighbour columns from the
// adjacent lanes with DPP wave shifts (no LDS, no barrier) and from two halo loads at the strip
// edges. All memory access goes through buffer descriptors with per-lane byte offsets, so a lane
// that has nothing to load carries an out-of-range offset instead of sitting behind an `if`:
// the loop bodies are branch-free and every load of a trip is in flight before the first use.
// Every HBM byte is touched by exactly one 16-byte access of one lane, plus the 3-row / 3-column
// halos that stay in the XCD's L2. Reflect-101 borders are register selects.
//
// The marches evaluate exactly the oracle's MUSICA_ORDER_FAST arithmetic.
#pragma once
#include <type_traits>
#include "kernels_common.h"
#include "sdev_parts.h"
#include "launchers.h"

namespace musica {

// Per-lane geometry of a 512-column strip, as byte offsets inside one row.
struct LaneCfg {
    int c;               // first fine column of this lane
    bool active;         // c < S
    bool left_mirror;    // lane 0 of the first strip: columns -2, -1 mirror onto 2, 1
    bool last_active;    // the lane holding column S-1: column S mirrors onto S-2
    bool lane0, lane63;
    uint32_t off;        // fine columns c .. c+7            (kOob when the lane is right of the image)
    uint32_t off_l;      // fine columns c-2, c-1            (lane 0 of a strip that is not the first, else kOob)
    uint32_t off_r;      // fine column  c+8                 (lane 63 with more image to its right, else kOob)
    uint32_t coff;       // coarse columns c/2 .. c/2+3
    uint32_t coff_l;     // coarse column  c/2-1
    uint32_t coff_r;     // coarse column  c/2+4
};

__device__ __forceinline__ LaneCfg make_cfg(int strip, int lane, int S) {
    LaneCfg g;
    const int c0 = strip * kStripCols;
    g.c = c0 + lane * kLaneCols;
    g.active = g.c < S;
    g.lane0 = lane == 0;
    g.lane63 = lane == 63;
    const bool left_load = g.lane0 && c0 > 0;
    const bool right_load = g.lane63 && (g.c + kLaneCols < S);
    g.left_mirror = g.lane0 && c0 == 0;
    g.last_active = g.active && (g.c + kLaneCols >= S);
    g.off = g.active ? (uint32_t)g.c * 4u : kOob;
    g.off_l = left_load ? (uint32_t)(g.c - 2) * 4u : kOob;
    g.off_r = right_load ? (uint32_t)(g.c + kLaneCols) * 4u : kOob;
    g.coff = g.active ? (uint32_t)(g.c >> 1) * 4u : kOob;
    g.coff_l = left_load ? (uint32_t)((g.c >> 1) - 1) * 4u : kOob;
    g.coff_r = right_load ? (uint32_t)((g.c >> 1) + 4) * 4u : kOob;
    return g;
}

__device__ __forceinline__ void load8(float d[8], const Buf& b, uint32_t off) {
    const float4 a = bload4(b, off), c = bload4(b, off + 16u);
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = c.x; d[5] = c.y; d[6] = c.z; d[7] = c.w;
}
__device__ __forceinline__ void store8_nt(const Buf& b, uint32_t off, const float d[8]) {
    bstore4_nt(b, off, make_float4(d[0], d[1], d[2], d[3]));
    bstore4_nt(b, off + 16u, make_float4(d[4], d[5], d[6], d[7]));
}

// ---- level 0 straight from the raw pixels ------------------------------------------------------
// The reference materialises sqrt and normalized images (6 + 8 B/px of traffic) before the pyramid
// starts. Here the level-0 kernels read the uint16 pixels (2 B/px) and apply img_sqrt.comp:15 +
// img_normalize.comp:24 to every pixel they load — the same three IEEE operations k_normalize executes,
// so the values are bit-identical — and the normalized image is only produced on demand.
__device__ __forceinline__ void norm8(float d[8], float4 m, const NormK& nk) {
    const uint32_t w[4] = {__float_as_uint(m.x), __float_as_uint(m.y), __float_as_uint(m.z), __float_as_uint(m.w)};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        d[2 * k] = norm_px(w[k] & 0xFFFFu, nk);
        d[2 * k + 1] = norm_px(w[k] >> 16, nk);
    }
}

// ======================================================================================
// Zero-inserted upsample + x4 smooth (K7 + K8) of a coarse image, shared by band and expand.
// Fine (x, y) on the S grid; coarse c on the Sc = ceil(S/2) grid.
//   V(j, y) : vertical pass on coarse column j      even y = 2k: (w0*c[km1] + w2*c[k]) + w4*c[kp1]
//                                                   odd  y     :  w1*c[k] + w3*c[kp1]
//   H(x, y) : horizontal pass on V                  even x = 2j: (w0*V[jm1] + w2*V[j]) + w4*V[jp1]
//                                                   odd  x     :  w1*V[j] + w3*V[jp1]
//   lowpass = 4 * H
// km1 / kp1 follow the reflect-101 mirror on the FINE grid (img_smooth_upsampled.comp:10-16).
// ======================================================================================

// Coarse index hit by fine tap index f after mirroring, or -1 when the tap reads a zero
// (odd texel, Q2) or leaves the image (Q1).
__device__ __forceinline__ int coarse_of_fine(int f, int S) {
    const int m = mirror_idx(f, S - 1);
    if (m < 0 || m >= S || (m & 1)) return -1;
    return m >> 1;
}

struct CRow {
    float v[4];  // coarse columns j0 .. j0+3
    float hl;    // coarse column j0-1 (lane 0 of a strip that is not the first)
    float hr;    // coarse column j0+4 (lane 63 with more image to its right)
};

__device__ __forceinline__ void load_crow(CRow& r, const Buf& b, uint32_t row_off, const LaneCfg& g) {
    const float4 a = bload4(b, g.coff + row_off);
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    // one halo column per edge lane: lane 0 reads j0-1, lane 63 reads j0+4 (every other lane carries kOob on both) — one load, one register;
    // hl and hr hold the same value and the two chains the callers build on them are one
    r.hl = r.hr = bload1(b, (g.lane0 ? g.coff_l : g.coff_r) + row_off);
}
// load_crow() of a trip that may not exist: without `more` (wave-uniform) it requests out of range — no traffic
__device__ __forceinline__ void load_crow_if(CRow& r, const Buf& b, uint32_t row_off, const LaneCfg& g, bool more) {
    const float4 q = bload4(b, (more ? g.coff : kOob) + row_off);
    r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    r.hl = r.hr = bload1(b, (more ? (g.lane0 ? g.coff_l : g.coff_r) : kOob) + row_off);
}

// Horizontal pass for the 8 fine columns of a lane from its 4 coarse V values + neighbours; returns 4 * H.
__device__ __forceinline__ void hpass8(const float V[4], float Vl, float Vr, float low[8]) {
    low[0] = 4.0f * chain_even(Vl, V[0], V[1]);
    low[1] = 4.0f * chain_odd(V[0], V[1]);
    low[2] = 4.0f * chain_even(V[0], V[1], V[2]);
    low[3] = 4.0f * chain_odd(V[1], V[2]);
    low[4] = 4.0f * chain_even(V[1], V[2], V[3]);
    low[5] = 4.0f * chain_odd(V[2], V[3]);
    low[6] = 4.0f * chain_even(V[2], V[3], Vr);
    low[7] = 4.0f * chain_odd(V[3], Vr);
}

// Neighbour exchange for one row of V values (S % 8 == 0, so S is even and the fine column S
// mirrors onto S-2 = coarse j0+3 of the last active lane; fine column -2 mirrors onto coarse 1).
__device__ __forceinline__ void exchange(const float V[4], float Vhl, float Vhr, const LaneCfg& g, float& Vl, float& Vr) {
    Vl = from_left_lane(V[3]);
    Vr = from_right_lane(V[0]);
    if (g.lane0) Vl = g.left_mirror ? V[1] : Vhl;
    if (g.last_active) Vr = V[3];
    else if (g.lane63) Vr = Vhr;
}

// Lowpass rows 2k and 2k+1 (8 fine columns each) from coarse rows a = km1, b = k, c = kp1.
__device__ __forceinline__ void lowpass_pair(const CRow& a, const CRow& b, const CRow& c, const LaneCfg& g,
                                             float lowE[8], float lowO[8]) {
    float Ve[4], Vo[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        Ve[j] = chain_even(a.v[j], b.v[j], c.v[j]);
        Vo[j] = chain_odd(b.v[j], c.v[j]);
    }
    const float Vehl = chain_even(a.hl, b.hl, c.hl), Vohl = chain_odd(b.hl, c.hl);
    const float Vehr = chain_even(a.hr, b.hr, c.hr), Vohr = chain_odd(b.hr, c.hr);
    float l, r;
    exchange(Ve, Vehl, Vehr, g, l, r);
    hpass8(Ve, l, r, lowE);
    exchange(Vo, Vohl, Vohr, g, l, r);
    hpass8(Vo, l, r, lowO);
}

// ======================================================================================
// Level 0 in one march: K1 + K4 + K5 + K6 and K7 + K8 + K9 — smooth + downsample AND the band-pass image — from one read
// of the fine image. As two launches, a reduce and a band kernel on the raw pixels each read and normalise the whole image
// (2 x (2 B/px + ~14 instructions per pixel)) and the band launch reads the coarse image back (1 B/px); here a wavefront
// that marches down its strip keeps the last three coarse rows it produced in registers and emits the band rows 2k, 2k+1
// as soon as coarse row k+1 exists: 7 B/px instead of 3 + 7, one launch instead of two.
// What a strip cannot take from its neighbours' registers it recomputes: the coarse rows k0-1 and k1 above / below its
// segment (two extra fine rows at either end) and, on lane 0 / lane 63, the coarse column left / right of the strip
// (four raw halo pixels per row instead of two / one). Every value is produced by the expressions of reduce_row()
// (kernels_pyramid.hip) and lowpass_pair(), so both outputs are bit-identical to the two-kernel path (tested against the oracle and against it).
// ======================================================================================
// Level 0 (raw pixels, FRowQ): the four halo pixels are requested by the edge lane alone, one 8-byte request per row, and then spread over the
// four lanes of its quad in registers (edge_quad_word): lane i of the first quad normalises column c0-4+i and runs its vertical chain, lane 60+i
// of the last quad column c0+512+i — one norm_px and one chain5 per lane and row where every lane ran four — and coarse_row() gathers the
// four chains back with quad broadcasts. (Round 4 had spread the columns by LOADING one per lane: eight 2-byte requests per row instead of two
// 8-byte ones, the same 49 - 53 us at 8 x 2048^2 and 96 - 115 us instead of 89 - 91 us at 8192^2. profiles/r04_rb0_experiments.txt)
// The f32 levels keep the four halo values on every lane (FRow): there is no normalisation to save, and spreading four whole words costs
// more moves than the three chains it removes (319 -> 331 vector instructions per trip, profiles/r06_level0_lane_work.txt).
struct FRow {
    float v[8];   // pixels c .. c+7
    float h[4];   // c-4 .. c-1 on lane 0, c+8 .. c+11 on lane 63 (strips with a neighbour on that side; 0 elsewhere)
};
struct FRowQ {
    float v[8];   // normalized pixels c .. c+7
    float h;      // lane i of the strip's first quad: column c0-4+i; lane 60+i: column c0+512+i (strips with a neighbour on that side); unused elsewhere
};
struct RawF {
    float4 m;     // 8 raw uint16 (bit pattern)
    float2 h;     // 4 raw halo pixels
};
__device__ __forceinline__ void load_raw_f(RawF& r, const Buf& b, uint32_t row_off, uint32_t off, uint32_t off_h) {
    r.m = bload4(b, off + row_off);
    r.h = bload2(b, off_h + row_off);
}
// `qi` = lane % 4: which of the edge lane's four halo pixels this lane takes
__device__ __forceinline__ void convert_f(FRowQ& r, const RawF& w, const NormK& nk, const uint32_t qi) {
    norm8(r.v, w.m, nk);
    const uint32_t a = edge_quad_word(__float_as_uint(w.h.x)), b = edge_quad_word(__float_as_uint(w.h.y));
    r.h = norm_px(((qi & 2u) ? b : a) >> ((qi & 1u) * 16u) & 0xFFFFu, nk);
}
// One coarse row (the lane's 4 columns + the halo column of an edge lane) from its five fine rows: reduce_row()'s arithmetic.
// the vertical chains of the four halo columns, as lane 0 / lane 63 use them
__device__ __forceinline__ void halo_chains(float (&vh)[4], const FRow& r0, const FRow& r1, const FRow& r2, const FRow& r3, const FRow& r4) {
#pragma unroll
    for (int j = 0; j < 4; j++) vh[j] = chain5(r0.h[j], r1.h[j], r2.h[j], r3.h[j], r4.h[j]);
}
// one chain per lane of the edge lane's quad (c-4 .. c-1 for lane 0, c+8 .. c+11 for lane 63), gathered with quad broadcasts
__device__ __forceinline__ void halo_chains(float (&vh)[4], const FRowQ& r0, const FRowQ& r1, const FRowQ& r2, const FRowQ& r3, const FRowQ& r4) {
    const float vq = chain5(r0.h, r1.h, r2.h, r3.h, r4.h);
    vh[0] = quad_bcast<0>(vq); vh[1] = quad_bcast<1>(vq); vh[2] = quad_bcast<2>(vq); vh[3] = quad_bcast<3>(vq);
}
template <class R>
__device__ __forceinline__ void coarse_row(CRow& cr, const R& r0, const R& r1, const R& r2, const R& r3, const R& r4, const LaneCfg& g) {
    float v[8], vh[4];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = chain5(r0.v[j], r1.v[j], r2.v[j], r3.v[j], r4.v[j]);
    halo_chains(vh, r0, r1, r2, r3, r4);
    float vl6 = from_left_lane(v[6]);
    float vl7 = from_left_lane(v[7]);
    float vr0 = from_right_lane(v[0]);
    if (g.lane0) {
        vl6 = g.left_mirror ? v[2] : vh[2];  // column -2 -> 2, -1 -> 1 (img_smooth.comp:13); else columns c-2, c-1
        vl7 = g.left_mirror ? v[1] : vh[3];
    }
    if (g.last_active) vr0 = v[6];           // column S -> S-2 (img_smooth.comp:12)
    else if (g.lane63) vr0 = vh[0];          // column c+8
    cr.v[0] = chain5(vl6, vl7, v[0], v[1], v[2]);
    cr.v[1] = chain5(v[0], v[1], v[2], v[3], v[4]);
    cr.v[2] = chain5(v[2], v[3], v[4], v[5], v[6]);
    cr.v[3] = chain5(v[4], v[5], v[6], v[7], vr0);
    // the coarse column next to the strip: j0-1 (fine c-4 .. c) on lane 0, j0+4 (fine c+6 .. c+10) on lane 63 — what the
    // neighbouring strip's edge lane computes as its own column
    const bool r = g.lane63;
    const float ch = chain5(r ? v[6] : vh[0], r ? v[7] : vh[1], r ? vh[0] : vh[2], r ? vh[1] : vh[3], r ? vh[2] : v[0]);
    cr.hl = ch;
    cr.hr = ch;
}
// Band rows 2k, 2k + 1 from coarse rows a = km1, b = k, c = kp1 and the fine rows fe, fo.
// SQ: for the march that also counts the level's noise histogram (reduce_band_block<true, true>): the pair is stored only where
// `store` (wave-uniform) says so — the pairs above and below a segment only feed the 5 x 5 sums — and its squares go into se / so. A lane
// right of the image normalises pixels it never loaded: its squares are 0, what img_sdev.comp reads there.
template <bool SQ = false, class R>
__device__ __forceinline__ void band_pair(const CRow& a, const CRow& b, const CRow& c, const R& fe, const R& fo, const LaneCfg& g,
                                          const Buf& bb, uint32_t off_e, uint32_t off_o, bool store = true, SRow* se = nullptr, SRow* so = nullptr) {
    float lowE[8], lowO[8], be[8], bo[8];
    lowpass_pair(a, b, c, g, lowE, lowO);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        be[j] = fe.v[j] - lowE[j];   // img_difference.comp:15
        bo[j] = fo.v[j] - lowO[j];
    }
    if (store) {
        store8_nt(bb, g.off + off_e, be);   // non-temporal: the band image is next read by another launch (C5 level 0: 108 -> 90 us)
        store8_nt(bb, g.off + off_o, bo);
    }
    if constexpr (SQ) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float te = g.active ? be[j] : 0.0f, to = g.active ? bo[j] : 0.0f;
            se->q[j] = te * te;
            so->q[j] = to * to;
        }
        se->e0 = se->e1 = so->e0 = so->e1 = 0.0f;   // the columns beside the strip are the seam pass's (hist_seam_block)
    }
}

// bit j: fe.v[j] <= 0.9, bit 8 + j: fo.v[j] <= 0.9 — the shader's own comparison on the normalized value (NaN: false)
__device__ __forceinline__ uint32_t le090_bits(const FRowQ& fe, const FRowQ& fo) {
    uint32_t m = 0u;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        m |= fe.v[j] <= 0.90f ? 1u << j : 0u;
        m |= fo.v[j] <= 0.90f ? 1u << (8 + j) : 0u;
    }
    return m;
}

__device__ __forceinline__ void load_f(FRow& r, const Buf& b, uint32_t row_off, uint32_t off, uint32_t off_h) {
    load8(r.v, b, off + row_off);
    const float4 h = bload4(b, off_h + row_off);
    r.h[0] = h.x; r.h[1] = h.y; r.h[2] = h.z; r.h[3] = h.w;
}

// rows_per_wave counts coarse rows. grid: x = strips, y = ceil(segments / 4), z = batch.
// U16: the fine image is the raw uint16 input, normalised on the fly (level 0); the two rows of the next trip are requested as
// raw pixels (6 registers) one trip ahead. Otherwise the fine image is f32 (levels >= 1): the rows are loaded where they are
// needed (a prefetch would cost 24 registers and a wavefront per SIMD; these levels are small and L2-resident).
// one workgroup of the launch: `tile` = its strip and block of four segments, `img` = its image (k_reduce_band, kernels_pyramid.hip; the paired launch of
// kernels_expand_sd.hip gives some of its workgroups this role)
// NH (level 0 only): the march also counts the level's noise histogram (img_sdev.comp + noise_hist.comp) from the band values it has in
// registers when it stores them, instead of a pass that reads the band image back. The wavefront keeps the squares of its last six band
// rows and, when band rows 2 kp, 2 kp + 1 exist, scans rows 2 kp - 2, 2 kp - 1 with sdev_row() — the arithmetic and the bookkeeping of
// every other form. It scans the rows of its own segment, so it computes one band pair more at either end than it stores (ks = k0 - 2,
// ke = k1 + 1: two more trips), and a segment holds whole 16-row runs (rows_per_wave % 8 == 0, the caller checks). Rows outside the
// image are zeros. The two columns either side of an interior strip boundary would need the neighbouring strip's band values: they
// start every run dead here and hist_seam_block() counts them from the stored band image. lh: the workgroup's cleared LDS histogram
// (the kernel flushes it); cov: the dispatch coverage of noise_hist.comp.
template <bool U16, bool NH = false>
__device__ __forceinline__ void reduce_band_block(const void* __restrict__ fine, float* __restrict__ down, float* __restrict__ band,
                                                  int S, int pitch, size_t plane, int Sc, int cpitch, size_t cplane,
                                                  int rows_per_wave, const uint32_t* __restrict__ minmax, int min_chain_exact,
                                                  uint16_t* __restrict__ le090, const Tile tile, const int img,
                                                  uint32_t* lh = nullptr, int cov = 0) {
    static_assert(!NH || U16, "the histogram form is level 0's");
    const int lane = threadIdx.x & 63;
    const int seg = __builtin_amdgcn_readfirstlane((int)(tile.segblock * kWavesPerBlock + (threadIdx.x >> 6)));   // wave-uniform: row arithmetic stays on the scalar unit
    const int k0 = seg * rows_per_wave;
    if (k0 >= Sc) return;  // wave-uniform
    const int k1 = min(k0 + rows_per_wave, Sc);
    NormK nk = make_norm(0.0f, 1.0f);
    if (U16) {
        float minv, maxv;
        chain_scalars(minmax, img, min_chain_exact, minv, maxv);
        nk = make_norm(minv, maxv);
    }
    const Buf ib = U16 ? make_buf(reinterpret_cast<const uint16_t*>(fine) + (size_t)img * S * S, (size_t)S * S * 2)
                       : make_buf(reinterpret_cast<const float*>(fine) + (size_t)img * plane, plane * 4);
    const Buf db = make_buf(down + (size_t)img * cplane, cplane * 4);
    const Buf bb = make_buf(band + (size_t)img * plane, plane * 4);
    const LaneCfg g = make_cfg(tile.strip, lane, S);
    // U16 with le090: one uint16 per lane and row pair, bit j / 8 + j = `normalized <= 0.9` (img_relevant.comp:58) of column c + j in the
    // even / odd row — the level-0 expand launch bins the gradation histogram with it instead of reading the raw pixels again
    const bool want_mask = U16 && le090 != nullptr;
    const Buf mb = want_mask ? make_buf(le090 + (size_t)img * Sc * (S / 8), (size_t)Sc * (S / 8) * 2) : bb;
    const uint32_t moff = g.off == kOob ? kOob : (uint32_t)g.c >> 2, mrb = (uint32_t)S >> 2;
    // own pixels and four halo pixels: c-4 .. c-1 (lane 0 of a strip that is not the first) or c+8 .. c+11 (lane 63 with more image to its right)
    const uint32_t px_bytes = U16 ? 2u : 4u;
    const uint32_t foff = g.off == kOob ? kOob : (uint32_t)g.c * px_bytes;
    const uint32_t foff_h = g.off_l != kOob ? (uint32_t)(g.c - 4) * px_bytes : (g.off_r != kOob ? (uint32_t)(g.c + 8) * px_bytes : kOob);
    const uint32_t qi = (uint32_t)lane & 3u;
    const int hi = S - 1;
    const uint32_t frb = U16 ? (uint32_t)S * 2u : (uint32_t)pitch * 4u, rb = (uint32_t)pitch * 4u, crb = (uint32_t)cpitch * 4u;
    const int ks = max(k0 - (NH ? 2 : 1), 0), ke = min(k1 + (NH ? 1 : 0), Sc - 1);   // coarse rows this wavefront computes (the first / last only feed its band rows)

    typename std::conditional<U16, FRowQ, FRow>::type w0, w1, w2, w3, w4;
    RawF ra, rc;
    if constexpr (U16) {
        load_raw_f(ra, ib, (uint32_t)mirror_idx(2 * ks - 2, hi) * frb, foff, foff_h);
        convert_f(w0, ra, nk, qi);
        load_raw_f(ra, ib, (uint32_t)mirror_idx(2 * ks - 1, hi) * frb, foff, foff_h);
        convert_f(w1, ra, nk, qi);
        load_raw_f(ra, ib, (uint32_t)(2 * ks) * frb, foff, foff_h);
        convert_f(w2, ra, nk, qi);
        load_raw_f(ra, ib, (uint32_t)mirror_idx(2 * ks + 1, hi) * frb, foff, foff_h);
        load_raw_f(rc, ib, (uint32_t)mirror_idx(2 * ks + 2, hi) * frb, foff, foff_h);
    } else {
        load_f(w0, ib, (uint32_t)mirror_idx(2 * ks - 2, hi) * frb, foff, foff_h);
        load_f(w1, ib, (uint32_t)mirror_idx(2 * ks - 1, hi) * frb, foff, foff_h);
        load_f(w2, ib, (uint32_t)(2 * ks) * frb, foff, foff_h);
    }
    CRow c0, cm1, cm2;
    cm1 = CRow(); cm2 = CRow();
    // NH: q0 .. q5 = the squares of band rows 2 kp - 4 .. 2 kp + 1 once pair kp is in (q4, q5); zeros above row 0
    [[maybe_unused]] SRow q0 = SRow(), q1 = SRow(), q2 = SRow(), q3 = SRow(), q4 = SRow(), q5 = SRow();
    [[maybe_unused]] unsigned long long alive[8], start[8];
    [[maybe_unused]] const SCfg sg = make_scfg(tile.strip, lane, S);
    if constexpr (NH) {
        sdev_start_masks(start, alive, sg, cov);
        // columns c0, c0 + 1 of a strip with a left neighbour and c0 + 510, c0 + 511 of one with a right neighbour: the seam pass's
        const unsigned long long keep_l = tile.strip > 0 ? ~1ull : ~0ull, keep_r = (tile.strip + 1) * kStripCols < S ? ~(1ull << 63) : ~0ull;
        start[0] &= keep_l; start[1] &= keep_l; start[6] &= keep_r; start[7] &= keep_r;
    }
    // band rows 2 kq, 2 kq + 1 (their five-row neighbourhoods are complete once pair kq + 1 is in) and the window's step of two rows
    [[maybe_unused]] auto scan_pair = [&](int kq) {
        if (kq >= k0 && kq < k1) {  // wave-uniform
            sdev_row<true, true>(q0, q1, q2, q3, q4, sg, S, 2 * kq, cov, nullptr, bb, 0u, lh, alive, start, false);
            sdev_row<true, true>(q1, q2, q3, q4, q5, sg, S, 2 * kq + 1, cov, nullptr, bb, 0u, lh, alive, start, false);
        }
        q0 = q2; q1 = q3; q2 = q4; q3 = q5;
    };
    for (int k = ks; k <= ke; k++) {
        if constexpr (U16) {
            convert_f(w3, ra, nk, qi);   // the pair requested one trip ago
            convert_f(w4, rc, nk, qi);
            const int kn = min(k + 1, ke);
            load_raw_f(ra, ib, (uint32_t)mirror_idx(2 * kn + 1, hi) * frb, foff, foff_h);
            load_raw_f(rc, ib, (uint32_t)mirror_idx(2 * kn + 2, hi) * frb, foff, foff_h);
        } else {
            load_f(w3, ib, (uint32_t)mirror_idx(2 * k + 1, hi) * frb, foff, foff_h);
            load_f(w4, ib, (uint32_t)mirror_idx(2 * k + 2, hi) * frb, foff, foff_h);
        }
        coarse_row(c0, w0, w1, w2, w3, w4, g);
        if (k >= k0 && k < k1)  // wave-uniform
            bstore4_nt(db, g.coff + (uint32_t)k * crb, make_float4(c0.v[0], c0.v[1], c0.v[2], c0.v[3]));
        // coarse row k completes the neighbourhood of row k-1: band rows 2(k-1), 2(k-1)+1 are the two oldest rows of the window.
        // km1(0) = coarse_of_fine(-2) = 1 (reflect-101 on the fine grid, img_smooth_upsampled.comp:10-16): row k itself.
        const int kp = k - 1;
        if constexpr (NH) {
            if (kp >= max(k0 - 1, 0)) {  // wave-uniform; kp <= min(k1, Sc - 2) by ke
                const bool mine = kp >= k0 && kp < k1;
                if (want_mask && mine) bstore_u16(mb, moff + (uint32_t)kp * mrb, le090_bits(w0, w1));
                band_pair<true>(kp == 0 ? c0 : cm2, cm1, c0, w0, w1, g, bb, (uint32_t)(2 * kp) * rb, (uint32_t)(2 * kp + 1) * rb, mine, &q4, &q5);
                scan_pair(kp - 1);
            }
        } else if (kp >= k0 && kp < k1) {  // wave-uniform
            if constexpr (U16) if (want_mask) bstore_u16(mb, moff + (uint32_t)kp * mrb, le090_bits(w0, w1));
            band_pair(kp == 0 ? c0 : cm2, cm1, c0, w0, w1, g, bb, (uint32_t)(2 * kp) * rb, (uint32_t)(2 * kp + 1) * rb);
        }
        cm2 = cm1; cm1 = c0;
        w0 = w2; w1 = w3; w2 = w4;
    }
    // the last row pair of the image: kp1(Sc-1) = coarse_of_fine(S) = Sc-1 (fine row S mirrors onto S-2)
    if (k1 == Sc) {
        if constexpr (U16) if (want_mask) bstore_u16(mb, moff + (uint32_t)(Sc - 1) * mrb, le090_bits(w0, w1));
        if constexpr (NH) {
            band_pair<true>(cm2, cm1, cm1, w0, w1, g, bb, (uint32_t)(2 * (Sc - 1)) * rb, (uint32_t)(2 * (Sc - 1) + 1) * rb, true, &q4, &q5);
            scan_pair(Sc - 2);
            q4 = SRow(); q5 = SRow();   // rows S, S + 1: zeros
            scan_pair(Sc - 1);
        } else {
            band_pair(cm2, cm1, cm1, w0, w1, g, bb, (uint32_t)(2 * (Sc - 1)) * rb, (uint32_t)(2 * (Sc - 1) + 1) * rb);
        }
    }
}

// ======================================================================================
// K14 + K16 + K7 + K8 + K17: recon = lowpass(prev) + band * gain(sdev) [* nr(cnr)]
// ======================================================================================

// linearFunction() of noise_reduction.comp:24-31 with its slope m = (p2.y - p1.y) / (p2.x - p1.x) precomputed.
// selects, not branches (a NaN c fails both tests and yields m * NaN + lowFactor = NaN, like the if / else chain)
__device__ __forceinline__ float nr_factor_m(float c, float lowCnr, float lowFactor, float highCnr, float highFactor, float m) {
    float r = m * c + lowFactor;
    r = c > highCnr ? highFactor : r;
    r = c < lowCnr ? lowFactor : r;
    return r;
}

template <int GAIN>
__device__ __forceinline__ float gain_of(float s, float high, const CurveLds& t) {
    if (GAIN == GAIN_CONST) return high;
    if (GAIN == GAIN_RANGE) {
        if (s == 0.0f) return high;                          // points[0].x == x
        if (s >= 0.0f && s <= 1.0f) return 0.0f * s + high;  // m = (high - high) / (1 - 0) = 0
        return 0.0f;
    }
    return curve_eval(t, s);
}

// The streaming kernel's form of getY() for the 33-point contrast polyline (DevCurveLut): two 16-byte LDS reads and
// no branch — musica_lut_eval (curve_lut.h). Exactly curve_eval()'s result for every float s:
//   * s is first clamped with sf = min(s, 2): NaN becomes 2 (v_min_f32 returns the other operand), as do +inf and every
//     s > 2; all of them lie above x[32] = 1, where getY() matches no interval and returns 0 — and so does the table
//     (j = 33, segment {0, 0, 0});
//   * j = #{x[i] < sf} from the entry of sf's bit pattern (musica_device.h); j in 1..32 -> the interval [x[j-1], x[j]];
//   * j = 0 means sf <= x[0] = 0: getY() returns y[0] for sf == 0 (also -0) and 0 for negative sf.
// Degenerate curves (lut.ok == 0) take curve_eval()'s literal scan.
struct LutLds {
    float4 bucket[kLutCap];
    float4 seg[kLutPoints + 1];
    int32_t base;
    uint32_t ok;
};
// LUTOK is wave-uniform and decided once per wavefront (k_expand_fast picks the instantiation of the whole march): a per-texel
// `if (!ok) slow()` put a divergent branch and a call sequence around each of the 16 lookups of a trip. `base` is lut.base in a
// scalar register.
// NONNEG: s comes out of musica_rms25_8 (the SD march), never out of a stored image: musica_lut_eval_nonneg has the proof.
template <bool LUTOK, bool NONNEG = false>
__device__ __forceinline__ float curve_eval_lut(const CurveLds& t, const LutLds& lut, int base, float s) {
    if (!LUTOK) return curve_eval(t, s);
    if (NONNEG) return musica_lut_eval_nonneg(lut.bucket, lut.seg, base, s);
    return musica_lut_eval(lut.bucket, lut.seg, base, s);
}

// GH (level 0 only): the launch also accumulates the gradation histogram — img_relevant.comp + gradation_histogram.comp —
// of the texels it reconstructs, while they are still in registers (the reference re-reads the whole image for it).
// The reference's thread walks a 16 x 16 area and `return`s at the first texel that is exactly 0
// (gradation_histogram.comp:24); here every texel is binned and a zero only raises the image's gzero word: the literal
// kernel (k_grad_hist) then recounts that image into a second histogram and k_grad_curve takes that one. The relevance
// weight uint(relevant * 100) is the one k_grad_hist computes: one cnr classification per lane and row pair (the cnr scale
// is 8 here, so a lane's 8 columns and both rows of a pair sit under one cnr texel), `normalized <= 0.9` on the raw pixel.
// `normalized <= 0.9` comes as the bit image k_reduce_band<true> wrote (2 bytes per lane and row pair; the raw-pixel form, 32 bytes
// against the threshold thr090, left in round 4).
// CNR48: the cnr scale is 4 or 8 (levels 1 and 0 of every image side that is a multiple of 8): columns c..c+3 and c+4..c+7 of a
// lane each sit under one cnr texel. Wave-uniform like LUTOK and chosen the same way (the other form divides per texel).
// CH (with GH, CLAHE contexts): the launch also accumulates clahe_histogram.comp:13-45 — hist[tx][ty][bin] += 1 where
// relevant == 1.0 — of the texels it reconstructs (k_clahe_hist<true> re-read the whole reconstruction and the raw pixels for it:
// 36 us for one 4096^2 image). relevant == 1.0 is relevant_of()'s value spelled out: inside the border and either the ramp
// value ((r*r)*(r*r))*r itself 1.0 or cnr in [6, 256] with `normalized <= 0.9`. A workgroup's 512 columns and its rows touch at
// most 2 x 2 tiles (the launcher checks: tile side >= 512 and >= the workgroup's rows): lc = 2 copies x 4 tile slots x 256 bins.
constexpr int kChSlots = 4, kChCopies = 2;
// GH: four bank-staggered copies of the histogram (lane l adds into copy l % 4, see sdev_parts.h: neighbouring texels share bins,
// and lanes of one ds_add that hit the same address are served one after the other); the words below bin 0 and above bin 1023 of a copy
// take what is out of range (word 0 of the array is the first copy's lower one)
constexpr int kGhCopies = 4, kGhStride = MUSICA_GRAD_BINS + 8;
// SD (levels 0 .. 2 of a context that does not store their sdev images): the launch computes the 5 x 5 RMS of the band image itself, from a
// window of six band rows it keeps in registers — the bits k_sdev_hist would have stored (the same sum5 / musica_rms25_8 on the same
// squares, sdev_parts.h) — instead of reading them: 4 B per texel less to read here and 4 B less for the sdev launch to write.
struct BRow {
    float v[8];     // band columns c .. c+7
    float e0, e1;   // lane 0: columns c-2, c-1; lane 63: columns c+8, c+9 (0 where the image ends); unused elsewhere
};
__device__ __forceinline__ void sdev_from_band(const BRow& r0, const BRow& r1, const BRow& r2, const BRow& r3, const BRow& r4, float (&s)[8]) {
    float q[8];
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = sum5(r0.v[j] * r0.v[j], r1.v[j] * r1.v[j], r2.v[j] * r2.v[j], r3.v[j] * r3.v[j], r4.v[j] * r4.v[j]);
    const float qe0 = sum5(r0.e0 * r0.e0, r1.e0 * r1.e0, r2.e0 * r2.e0, r3.e0 * r3.e0, r4.e0 * r4.e0);
    const float qe1 = sum5(r0.e1 * r0.e1, r1.e1 * r1.e1, r2.e1 * r2.e1, r3.e1 * r3.e1, r4.e1 * r4.e1);
    const float a6 = from_left_lane_or(q[6], qe0), a7 = from_left_lane_or(q[7], qe1);   // lane 0 keeps its left pair, lane 63 its right one
    const float b0 = from_right_lane_or(q[0], qe0), b1 = from_right_lane_or(q[1], qe1);
    s[0] = sum5(a6, a7, q[0], q[1], q[2]);
    s[1] = sum5(a7, q[0], q[1], q[2], q[3]);
    s[2] = sum5(q[0], q[1], q[2], q[3], q[4]);
    s[3] = sum5(q[1], q[2], q[3], q[4], q[5]);
    s[4] = sum5(q[2], q[3], q[4], q[5], q[6]);
    s[5] = sum5(q[3], q[4], q[5], q[6], q[7]);
    s[6] = sum5(q[4], q[5], q[6], q[7], b0);
    s[7] = sum5(q[5], q[6], q[7], b0, b1);
    musica_rms25_8(s);
}
// Bits 0 .. 3 of x as the low bits of bytes 0 .. 3: the product moves bit i to i, i + 7, i + 14 and i + 21 — sixteen different places,
// so nothing carries — and bit 8k is reached from i = k alone.
__device__ __forceinline__ uint32_t spread4(uint32_t x) { return ((x & 15u) * 0x204081u) & 0x01010101u; }   // 4 x 22 bits: a 24-bit multiply
template <int GAIN, bool NR, bool GH, bool LUTOK, bool CNR48, bool CH = false, bool SD = false>
__device__ __forceinline__ bool expand_march(const ExpandArgs& a, const CurveLds& tab, const LutLds& lut, uint32_t* lh, int img, uint32_t* lc = nullptr,
                                             uint32_t tx0 = 0u, uint32_t ty0 = 0u) {
    // slope of noise_reduction.comp:28, the same value for every texel
    const float nr_m = (a.highFactor - a.lowFactor) / (a.highCnr - a.lowCnr);
    const int lane = threadIdx.x & 63;
    const Tile tile = xcd_tile(a.swz);
    const int seg = __builtin_amdgcn_readfirstlane((int)(tile.segblock * kWavesPerBlock + (threadIdx.x >> 6)));   // wave-uniform: row arithmetic stays on the scalar unit
    const int k0 = seg * a.rows_per_wave;
    bool saw_zero = false;
    const int lut_base = (GAIN == GAIN_CURVE && LUTOK) ? __builtin_amdgcn_readfirstlane(lut.base) : 0;   // one LDS word: wave-uniform
    if (k0 < a.Sc) {   // wave-uniform
    const int k1 = min(k0 + a.rows_per_wave, a.Sc);
    const int S = a.S;
    const int cnrScale = GH ? 8 : a.cnrScale;   // the launcher takes the GH variant only at scale 8
    const Buf bb = make_buf(a.band + (size_t)img * a.plane, a.plane * 4);
    const Buf sb = make_buf((GAIN != GAIN_CONST ? a.sdev : a.band) + (size_t)img * a.plane, a.plane * 4);
    const Buf ob = make_buf(a.recon + (size_t)img * a.plane, a.plane * 4);
    const Buf pb = make_buf(a.prev + (size_t)img * a.cplane, a.cplane * 4);
    const Buf wb = !GH ? bb : make_buf(a.le090 + (size_t)img * a.Sc * (S / 8), (size_t)a.Sc * (S / 8) * 2);   // `normalized <= 0.9` as k_reduce_band<true>'s bit image
    const float* cnr = NR ? a.cnr + (size_t)img * a.cnrPlane : nullptr;
    const LaneCfg g = make_cfg(tile.strip, lane, S);
    const uint32_t rb = (uint32_t)a.pitch * 4u, crb = (uint32_t)a.cpitch * 4u;
    const uint32_t moff = g.off == kOob ? kOob : (uint32_t)g.c >> 2, mrb = (uint32_t)S >> 2;
    // noise reduction: the 8 columns of a lane share ceil(8 / scale) cnr texels per row
    const int cxs[2] = {g.active ? g.c / cnrScale : 0, g.active ? (g.c + 4) / cnrScale : 0};
    // gradation histogram: img_relevant.comp:46-49 in uint arithmetic (wraps for N < 100 like the shader)
    const uint32_t border = 100u, lim = (uint32_t)S - border;
    uint32_t colin = 0u;
    if (GH) {
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (g.active && (uint32_t)(g.c + j) > border && (uint32_t)(g.c + j) < lim) colin |= 1u << j;
    }
    // the border bits as bytes of 0 / 1, four columns per word: the low half of row_phase's byte selectors, the same for every row of the lane
    const uint32_t colsp[2] = {spread4(colin & 15u), spread4(colin >> 4)};
    uint32_t* lhc = lh + (GH ? 1 + (lane & (kGhCopies - 1)) * kGhStride : 0);   // bin 0 of the lane's copy; the word below it is a spare one too
    // CLAHE tile column of each of the lane's 8 columns, relative to the workgroup's first one (clahe_histogram.comp:34)
    const float fS = (float)S;
    uint32_t chx = 0u;
    if (CH) {
#pragma unroll
        for (int j = 0; j < 8; j++) chx |= (min(f2u((float)(g.c + j) / fS * (float)MUSICA_CLAHE_TILES) - tx0, 1u)) << j;
    }
    uint32_t* lcc = CH ? lc + (lane & (kChCopies - 1)) * (kChSlots * MUSICA_CLAHE_BINS) : nullptr;

    // One row of a pair once its operands are in registers: contrast gain, noise reduction, addition, store, histograms.
    // `src` is the band row, `b` the registers the reconstructed row is left in (the same array, or — SD — the lowpass row's: the band row stays
    // in the window)
    auto row_phase = [&](const int ph, float* b, const float* src, const float* sd, const float* low, const float* f, const uint32_t le_t,
                         const int kk, const uint32_t wpair, const bool one_ramp, const bool one_dark) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            // contrast_curve_apply.comp:61
            float p = src[j] * (GAIN == GAIN_CURVE ? curve_eval_lut<LUTOK, SD>(tab, lut, lut_base, sd[j]) : gain_of<GAIN>(GAIN != GAIN_CONST ? sd[j] : 0.0f, a.high, tab));
            if (NR) p = p * f[j];   // noise_reduction.comp:57
            b[j] = low[j] + p;      // img_addition.comp:15
        }
        store8_nt(ob, g.off + (uint32_t)(2 * kk + ph) * rb, b);   // non-temporal since round 4: with steps in flight -2 % per step at 8 x 2048^2 (k_grad_apply has the numbers)
        if (GH) {
            const uint32_t dark = le_t >> (8 * ph);
            const uint32_t y = (uint32_t)(2 * kk + ph);
            const bool rowin = y > border && y < lim;                  // wave-uniform
            const uint32_t m = rowin ? colin : 0u;   // inside-the-border bits of the lane's 8 columns in this row (CH)
            // :28-30 uint(relevant * 100) of the row's 8 texels, once per row: 0 outside the border, w_cnr for a bright pixel inside it,
            // w_dark_or_ramp for a dark one — a byte each (all <= 100), picked out of wrow = {0, w_cnr, 0, w_dark_or_ramp} by the byte
            // selector (inside-the-border bit) + 2 * (`<= 0.9` bit); outside the border rows wrow is 0 altogether.
            const uint32_t wrow = rowin ? wpair : 0u;
            uint32_t wq[2];
#pragma unroll
            for (int h = 0; h < 2; h++) wq[h] = __builtin_amdgcn_perm(wrow, wrow, (spread4((le_t >> (8 * ph + 4 * h)) & 15u) << 1) | colsp[h]);
            const uint32_t chy = CH ? min(f2u((float)y / fS * (float)MUSICA_CLAHE_TILES) - ty0, 1u) : 0u;   // clahe_histogram.comp:35 (wave-uniform)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float cur = b[j];
                saw_zero = saw_zero || (cur == 0.0f);                        // gradation_histogram.comp:24
                // :26 int(cur * 1024) with "NaN never indexes" (oracle Q6) and "bins outside [0, 1024) are dropped" (Q1) folded into
                // the clamp: max(NaN, -1) = -1 and every scaled <= -1 land on the spare word below bin 0, everything >= 1024 on the spare
                // word above bin 1023 (neither is flushed); (-1, 0) truncates to bin 0 like the shader's int(). The clamped value indexes directly.
                const int bin = (int)fminf(fmaxf(cur * (float)MUSICA_GRAD_BINS, -1.0f), (float)MUSICA_GRAD_BINS);
                // adding 0 leaves the histogram as it is
                const bool le090 = CH && ((dark >> j) & 1u) != 0u;
                const uint32_t w = (wq[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                atomicAdd(&lhc[bin], w);
                if (CH) {
                    const float scaled = cur * (float)(MUSICA_CLAHE_BINS - 1) + 0.5f;                 // clahe_histogram.comp:20
                    const bool inrange = scaled > -1.0f && scaled < (float)MUSICA_CLAHE_BINS;       // NaN never indexes (Q6)
                    if (((m >> j) & 1u) && inrange && (one_ramp || (one_dark && le090)))
                        atomicAdd(&lcc[((((chx >> j) & 1u) * 2u + chy) * MUSICA_CLAHE_BINS) + (uint32_t)(int)scaled], 1u);   // :39-44
                }
            }
        }
    };
    if constexpr (SD) {
        // rows 2k - 2 .. 2k + 3 of the band image: six slots that rotate by two rows per trip; three trips are spelled out per loop iteration so
        // that a slot is a fixed set of registers (no moves). A row outside the image is requested out of range (zeros: Q1).
        const uint32_t off_e = g.lane0 ? g.off_l : g.off_r;
        auto load_brow = [&](BRow& r, const int y, const bool wanted) __attribute__((always_inline)) {
            const uint32_t row_off = (wanted && y >= 0 && y < S) ? (uint32_t)y * rb : kOob;   // wave-uniform
            load8(r.v, bb, (g.off + row_off) | ((g.off | row_off) & kOob));
            const float2 e = bload2(bb, (off_e + row_off) | ((off_e | row_off) & kOob));
            r.e0 = e.x; r.e1 = e.y;
        };
        CRow c0, c1, cn;
        load_crow(c0, pb, (uint32_t)coarse_of_fine(2 * k0 - 2, S) * crb, g);
        load_crow(c1, pb, (uint32_t)k0 * crb, g);
        load_crow(cn, pb, (uint32_t)coarse_of_fine(2 * k0 + 2, S) * crb, g);
        uint32_t le = 0u;
        float cq[2] = {0.0f, 0.0f};
        auto load_cnr2 = [&](const int kk) __attribute__((always_inline)) {
            const size_t re = (size_t)((2 * kk) / cnrScale) * a.cnrPitch;
            cq[0] = cnr[re + cxs[0]]; cq[1] = cnr[re + cxs[1]];
        };
        if (NR && CNR48) load_cnr2(k0);
        BRow w0, w1, w2, w3, w4, w5;
        load_brow(w0, 2 * k0 - 2, true); load_brow(w1, 2 * k0 - 1, true); load_brow(w2, 2 * k0, true);
        load_brow(w3, 2 * k0 + 1, true); load_brow(w4, 2 * k0 + 2, true); load_brow(w5, 2 * k0 + 3, true);
        if (GH) le = bload_u16(wb, moff + (uint32_t)k0 * mrb);
        auto trip = [&](const int k, BRow& r0, BRow& r1, BRow& r2, BRow& r3, BRow& r4, BRow& r5) __attribute__((always_inline)) {
            const bool more = k + 1 < k1;                     // wave-uniform
            const int kn = k + 1;
            uint32_t le_n = 0u;
            if (GH) le_n = bload_u16(wb, (more ? moff : kOob) + (uint32_t)kn * mrb);
            float lowE[8], lowO[8];
            lowpass_pair(c0, c1, cn, g, lowE, lowO);
            c0 = c1; c1 = cn;
            load_crow_if(cn, pb, (uint32_t)coarse_of_fine(2 * kn + 2, S) * crb, g, more);   // the next trip's coarse row (k + 2's neighbourhood), a whole trip ahead
            float fe[8], fo[8];
            float cnr_pair = 0.0f;
            if (NR) {
                if (CNR48) {
                    cnr_pair = cq[0] * kMaxCnrValue;
                    const float e0 = nr_factor_m(cnr_pair, a.lowCnr, a.lowFactor, a.highCnr, a.highFactor, nr_m);
                    const float e1 = nr_factor_m(cq[1] * kMaxCnrValue, a.lowCnr, a.lowFactor, a.highCnr, a.highFactor, nr_m);
#pragma unroll
                    for (int j = 0; j < 8; j++) { fe[j] = j < 4 ? e0 : e1; fo[j] = fe[j]; }
                    load_cnr2(more ? kn : k);
                } else {
                    const size_t re = (size_t)((2 * k) / cnrScale) * a.cnrPitch, ro = (size_t)((2 * k + 1) / cnrScale) * a.cnrPitch;
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int cx = g.active ? (g.c + j) / cnrScale : 0;                 // noise_reduction.comp:39-45
                        fe[j] = nr_factor_m(cnr[re + cx] * kMaxCnrValue, a.lowCnr, a.lowFactor, a.highCnr, a.highFactor, nr_m);
                        fo[j] = nr_factor_m(cnr[ro + cx] * kMaxCnrValue, a.lowCnr, a.lowFactor, a.highCnr, a.highFactor, nr_m);
                    }
                }
            }
            const CnrClass kc = classify_cnr(cnr_pair);
            const uint32_t w_cnr = kc.ramp ? kc.w_ramp : 0u, w_dark_or_ramp = kc.ramp ? kc.w_ramp : (kc.high ? 100u : 0u);
            const uint32_t wpair = (w_cnr << 8) | (w_dark_or_ramp << 24);   // row_phase's byte table
            const float r6 = cnr_pair / 6.0f;
            const bool one_ramp = CH && kc.ramp && (((r6 * r6) * (r6 * r6)) * r6 == 1.0f);
            const bool one_dark = CH && !kc.ramp && kc.high;
            {   // even row 2k: window rows 2k - 2 .. 2k + 2, its band values are the centre row's
                float sd[8];
                sdev_from_band(r0, r1, r2, r3, r4, sd);
                row_phase(0, lowE, r2.v, sd, lowE, fe, le, k, wpair, one_ramp, one_dark);
            }
            load_brow(r0, 2 * k + 4, more);   // the slot of row 2k - 2 takes row 2k + 4 (the next trip's; nothing if there is none)
            {   // odd row 2k + 1: rows 2k - 1 .. 2k + 3
                float sd[8];
                sdev_from_band(r1, r2, r3, r4, r5, sd);
                row_phase(1, lowO, r3.v, sd, lowO, fo, le, k, wpair, one_ramp, one_dark);
            }
            load_brow(r1, 2 * k + 5, more);
            le = le_n;
        };
        for (int k = k0; k < k1; k += 3) {
            trip(k, w0, w1, w2, w3, w4, w5);
            if (k + 1 < k1) trip(k + 1, w2, w3, w4, w5, w0, w1);
            if (k + 2 < k1) trip(k + 2, w4, w5, w0, w1, w2, w3);
        }
        return saw_zero;
    }
    // The march is a software pipeline (round 4): while a wavefront computes one row of a pair, the operands of its NEXT row are in
    // flight — the odd row's band / sdev registers are requested before the even row is computed, the next trip's even row into the even
    // row's registers as soon as that row is stored, the next trip's coarse row into the registers of the coarse row that has just left
    // the window, the next trip's cnr texels where this trip's have been consumed. No register more than the form that requested a whole
    // trip at its top and waited for the first of them at once would need: 128 registers, 4 wavefronts per SIMD, no scratch (114 before).
    // A trip that does not exist (beyond k1) requests out of range: no traffic.
    CRow c0, c1, cn;
    load_crow(c0, pb, (uint32_t)coarse_of_fine(2 * k0 - 2, S) * crb, g);
    load_crow(c1, pb, (uint32_t)k0 * crb, g);
    load_crow(cn, pb, (uint32_t)coarse_of_fine(2 * k0 + 2, S) * crb, g);
    float be[8], bo[8], se[8], so[8];
    uint32_t le = 0u;   // the pair's `<= 0.9` bits (GH)
    // cnr texels of a trip (CNR48: scale 4 or 8): the left / right half of the lane's columns; rows 2k and 2k + 1 sit under the same
    // cnr row at an even scale ((2k) / s == (2k + 1) / s), so a pair needs two texels, not four
    float cq[2] = {0.0f, 0.0f};
    auto load_cnr2 = [&](const int kk) __attribute__((always_inline)) {
        const size_t re = (size_t)((2 * kk) / cnrScale) * a.cnrPitch;
        cq[0] = cnr[re + cxs[0]]; cq[1] = cnr[re + cxs[1]];
    };
    if (NR && CNR48) load_cnr2(k0);
    load8(be, bb, g.off + (uint32_t)(2 * k0) * rb);
    if (GAIN != GAIN_CONST) load8(se, sb, g.off + (uint32_t)(2 * k0) * rb);
    if (GH) le = bload_u16(wb, moff + (uint32_t)k0 * mrb);
    for (int k = k0; k < k1; k++) {
        const bool more = k + 1 < k1;                     // wave-uniform
        const int kn = k + 1;
        const uint32_t goff_n = more ? g.off : kOob;      // next trip's rows: the lane's columns, or nothing
        // the next pair's `<= 0.9` bits a whole trip ahead (2 bytes per lane): requested with the next even row they would make the
        // bottom of the loop wait for that row (the rotation le = le_n is a register move of a loaded value)
        uint32_t le_n = 0u;
        if (GH) le_n = bload_u16(wb, (more ? moff : kOob) + (uint32_t)kn * mrb);
        // the odd row of this trip: in flight while the even row is computed
        load8(bo, bb, g.off + (uint32_t)(2 * k + 1) * rb);
        if (GAIN != GAIN_CONST) load8(so, sb, g.off + (uint32_t)(2 * k + 1) * rb);
        float lowE[8], lowO[8];
        lowpass_pair(c0, c1, cn, g, lowE, lowO);
        c0 = c1; c1 = cn;
        load_crow_if(cn, pb, (uint32_t)coarse_of_fine(2 * kn + 2, S) * crb, g, more);   // the next trip's coarse row (k + 2's neighbourhood), a whole trip ahead
        float fe[8], fo[8];  // noise-reduction factors of the two rows
        float cnr_pair = 0.0f;   // cnr * 256 of the texel above this lane's row pair (GH: scale 8)
        if (NR) {
            if (CNR48) {  // columns c..c+3 and c+4..c+7 each sit inside one cnr texel (c % 8 == 0)
                cnr_pair = cq[0] * kMaxCnrValue;
                const float e0 = nr_factor_m(cnr_pair, a.lowCnr, a.lowFactor, a.highCnr, a.highFactor, nr_m);
                const float e1 = nr_factor_m(cq[1] * kMaxCnrValue, a.lowCnr, a.lowFactor, a.highCnr, a.highFactor, nr_m);
#pragma unroll
                for (int j = 0; j < 8; j++) { fe[j] = j < 4 ? e0 : e1; fo[j] = fe[j]; }
                load_cnr2(more ? kn : k);   // branch-free: the last trip asks for its own texels again
            } else {
                const size_t re = (size_t)((2 * k) / cnrScale) * a.cnrPitch, ro = (size_t)((2 * k + 1) / cnrScale) * a.cnrPitch;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int cx = g.active ? (g.c + j) / cnrScale : 0;                 // noise_reduction.comp:39-45
                    fe[j] = nr_factor_m(cnr[re + cx] * kMaxCnrValue, a.lowCnr, a.lowFactor, a.highCnr, a.highFactor, nr_m);
                    fo[j] = nr_factor_m(cnr[ro + cx] * kMaxCnrValue, a.lowCnr, a.lowFactor, a.highCnr, a.highFactor, nr_m);
                }
            }
        }
        // img_relevant.comp:44-63 for the cnr texel above the row pair (rows 2k, 2k+1 and columns c..c+7 share it)
        const CnrClass kc = classify_cnr(cnr_pair);
        const uint32_t w_cnr = kc.ramp ? kc.w_ramp : 0u, w_dark_or_ramp = kc.ramp ? kc.w_ramp : (kc.high ? 100u : 0u);   // bright / dark pixel under this texel
        const uint32_t wpair = (w_cnr << 8) | (w_dark_or_ramp << 24);   // row_phase's byte table
        // relevant == 1.0 (CH): the ramp value itself, else 1.0 for a dark pixel under a high-cnr texel (relevant_of)
        const float r6 = cnr_pair / 6.0f;
        const bool one_ramp = CH && kc.ramp && (((r6 * r6) * (r6 * r6)) * r6 == 1.0f);
        const bool one_dark = CH && !kc.ramp && kc.high;
        // (Left alone, the machine scheduler moves the first instructions on the odd row's operands — the NaN-quieting v_max of the
        // lookup — up into the even row's phase, and the wait for the odd row with them. __builtin_amdgcn_sched_barrier(0) in front of
        // either phase keeps them apart, and costs more than it saves: 153 registers, i.e. 84 bytes of scratch at 4 wavefronts per SIMD
        // (116 us) or 3 wavefronts per SIMD (85.9 us, the same as this form: 85.2 - 87.2 against 89.4 - 89.7 us before the pipeline).)
        row_phase(0, be, be, se, lowE, fe, le, k, wpair, one_ramp, one_dark);
        // the even row of the next trip into the registers the even row has just left
        load8(be, bb, goff_n + (uint32_t)(2 * kn) * rb);
        if (GAIN != GAIN_CONST) load8(se, sb, goff_n + (uint32_t)(2 * kn) * rb);
        row_phase(1, bo, bo, so, lowO, fo, le, k, wpair, one_ramp, one_dark);
        le = le_n;
    }
    }
    return saw_zero;
}

template <int GAIN, bool NR, bool GH, int W = 1, bool CH = false, bool SD = false>
__global__ __launch_bounds__(kBlockThreads, W) void k_expand_fast(ExpandArgs a) {
    __shared__ CurveLds tab;
    __shared__ __attribute__((aligned(16))) LutLds lut;
    __shared__ uint32_t lh[GH ? kGhCopies * kGhStride + 1 : 1];
    __shared__ uint32_t lc[CH ? kChCopies * kChSlots * MUSICA_CLAHE_BINS : 1];
    const int img = blockIdx.z;
    if (GH)
        for (int i = threadIdx.x; i < kGhCopies * kGhStride + 1; i += blockDim.x) lh[i] = 0u;
    uint32_t tx0 = 0u, ty0 = 0u;   // CLAHE tile of the workgroup's first column / first row
    if (CH) {
        for (int i = threadIdx.x; i < kChCopies * kChSlots * MUSICA_CLAHE_BINS; i += blockDim.x) lc[i] = 0u;
        const Tile t = xcd_tile(a.swz);
        tx0 = f2u((float)(t.strip * kStripCols) / (float)a.S * (float)MUSICA_CLAHE_TILES);
        ty0 = f2u((float)(t.segblock * kWavesPerBlock * a.rows_per_wave * 2) / (float)a.S * (float)MUSICA_CLAHE_TILES);
    }
    if (GAIN == GAIN_CURVE) {
        const DevCurve* cv = a.curves + (size_t)img * a.curve_stride;
        const DevCurveLut* lv = a.luts + (size_t)img * MUSICA_COARSER_LEVELS_START;
        curve_to_lds(tab, cv);
        const int nlut = lv->ok ? min((int)lv->n, kLutCap) : 0;   // only the entries in use (a few hundred for typical noise modes)
        for (int i = threadIdx.x; i < nlut; i += blockDim.x) lut.bucket[i] = lv->bucket[i];
        for (int i = threadIdx.x; i <= kLutPoints; i += blockDim.x) lut.seg[i] = lv->seg[i];
        if (threadIdx.x == 0) { lut.base = lv->base; lut.ok = lv->ok; }
        __syncthreads();
    }
    // wave-uniform (one LDS word): readfirstlane tells the compiler so, and the whole march is instantiated per case
    const bool lut_ok = GAIN != GAIN_CURVE || __builtin_amdgcn_readfirstlane((int)lut.ok) != 0;
    const bool cnr48 = !NR || GH || a.cnrScale == 4 || a.cnrScale == 8;   // kernel argument: uniform
    bool saw_zero;
    if (lut_ok && cnr48) saw_zero = expand_march<GAIN, NR, GH, true, true, CH, SD>(a, tab, lut, lh, img, lc, tx0, ty0);
    else if (lut_ok) saw_zero = expand_march<GAIN, NR, GH, true, NR && !GH ? false : true, CH, SD>(a, tab, lut, lh, img, lc, tx0, ty0);
    else if (cnr48) saw_zero = expand_march<GAIN, NR, GH, GAIN != GAIN_CURVE, true, CH, SD>(a, tab, lut, lh, img, lc, tx0, ty0);
    else saw_zero = expand_march<GAIN, NR, GH, GAIN != GAIN_CURVE, NR && !GH ? false : true, CH, SD>(a, tab, lut, lh, img, lc, tx0, ty0);
    if (GH) {
        if (saw_zero) atomicOr(&a.gzero[img], 1u);
        __syncthreads();
        uint32_t* gh = a.ghist + (size_t)img * MUSICA_GRAD_BINS;
        for (int i = threadIdx.x; i < MUSICA_GRAD_BINS; i += blockDim.x) {
            uint32_t v = 0u;
#pragma unroll
            for (int k = 0; k < kGhCopies; k++) v += lh[1 + k * kGhStride + i];
            if (v) atomicAdd(&gh[i], v);
        }
        if (CH) {
            uint32_t* ch = a.chist + (size_t)img * MUSICA_CLAHE_TILES * MUSICA_CLAHE_TILES * MUSICA_CLAHE_BINS;
            for (int i = threadIdx.x; i < kChSlots * MUSICA_CLAHE_BINS; i += blockDim.x) {
                const uint32_t slot = (uint32_t)i / MUSICA_CLAHE_BINS, tx = tx0 + (slot >> 1), ty = ty0 + (slot & 1u);
                uint32_t v = 0u;
#pragma unroll
                for (int k = 0; k < kChCopies; k++) v += lc[k * kChSlots * MUSICA_CLAHE_BINS + i];
                if (v && tx < (uint32_t)MUSICA_CLAHE_TILES && ty < (uint32_t)MUSICA_CLAHE_TILES)
                    atomicAdd(&ch[(tx * MUSICA_CLAHE_TILES + ty) * MUSICA_CLAHE_BINS + ((uint32_t)i % MUSICA_CLAHE_BINS)], v);
            }
        }
    }
}

// the grid of a streaming launch: x = strips, y = ceil(segments / 4), z = batch (`rows` rows in segments of rows_per_wave, one per wavefront)
static inline dim3 stream_grid(int S, int rows, int rows_per_wave, int batch) {
    const int strips = (S + kStripCols - 1) / kStripCols;
    const int segs = (rows + rows_per_wave - 1) / rows_per_wave;
    return dim3(strips, (segs + kWavesPerBlock - 1) / kWavesPerBlock, batch);
}

}  // namespace musica
