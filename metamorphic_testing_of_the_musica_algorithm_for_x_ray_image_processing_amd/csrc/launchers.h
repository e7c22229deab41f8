// launchers.h — host-callable launch wrappers implemented in the kernel files, plus the
// argument blocks they share with the host code: the step's launch sequence in musica_step.hip and the study's entry points in musica_study.hip.
#pragma once

#include <stdlib.h>
#include <vector>
#include "musica_device.h"

namespace musica {

// How the contrast gain of a level is obtained (contrast_curve_apply.comp:61 with the curve of
// contrast_curve_generate.comp:56-94):
//   GAIN_CONST : levels >= 4 — the sdev image is never written there (src/vk_processing.cpp:2285), so
//                getY(0) == points[0].y == highContrastFactor exactly;
//   GAIN_RANGE : level 3 — two-point constant curve but a real sdev: getY(s) = 0*s + high for
//                0 <= s <= 1 (== high for finite s), 0 for s > 1 or NaN;
//   GAIN_CURVE : levels 0..2 — the 33-point polyline.
enum { GAIN_CONST = 0, GAIN_RANGE = 1, GAIN_CURVE = 2 };

struct ExpandArgs {
    const float* prev;   // coarse reconstruction (or downsampled[L-1] for the first slot)
    const float* band;
    const float* sdev;   // GAIN_RANGE / GAIN_CURVE
    const float* cnr;    // noise reduction (levels 0, 1)
    float* recon;
    const DevCurve* curves;  // curve of this level for image 0 (GAIN_CURVE)
    const DevCurveLut* luts; // its bucket table (GAIN_CURVE), stride MUSICA_COARSER_LEVELS_START per image
    int S, pitch; size_t plane;
    int Sc, cpitch; size_t cplane;
    int cnrS, cnrPitch; size_t cnrPlane;
    int cnrScale;        // uint(ceil(S / float(cnrS))), noise_reduction.comp:38
    float high;          // highContrastFactor of the level
    float lowCnr, lowFactor, highCnr, highFactor;  // NoiseReductionParams of the level
    int rows_per_wave;
    size_t curve_stride; // DevCurve elements between consecutive images
    // Level 0 only, NULL otherwise: the launch also accumulates the gradation histogram (img_relevant.comp +
    // gradation_histogram.comp) of the texels it has just reconstructed, see k_expand_fast<.., GH = true>.
    const uint16_t* raw;     // raw pixels (dense rows of S): `normalized <= 0.9` is tested as raw <= thr090[image]
    uint32_t* ghist;         // [batch][1024]
    uint32_t* gzero;         // [batch]: set when a reconstructed texel is exactly 0 (the `return` of gradation_histogram.comp:24
                             // then cuts the scan of its 16 x 16 area short: k_grad_hist redoes that image literally)
    const uint16_t* le090;   // or: [batch][Sc][S / 8] bits of `normalized <= 0.9` written by launch_reduce_band_u16 (then raw / thr090 are not read)
    uint32_t* chist;         // CLAHE contexts, with le090: [batch][4][4][256], the launch also counts clahe_histogram.comp (k_expand_fast<.., CH = true>)
    int swz;                 // XCD-aware tile mapping (kernels_common.h xcd_tile)
    const int* thr090;       // [batch]: largest raw value whose normalized value is <= 0.9 (k_curves_cnr)
    int ref_order;           // generic kernels: the shaders' literal 25-tap order (MUSICA_FLAG_REFERENCE_ORDER)
};

struct GradArgs {
    const float* img;        // expandImageStates[L-1]: the contrast-enhanced image
    const float* normalized;
    const float* cnr;
    uint32_t* hist;          // [batch][1024]
    int N, pitch; size_t plane;
    int cnrS, cnrPitch; size_t cnrPlane;
    int cnrScale;            // uint(ceil(N / float(cnrS))), img_relevant.comp:32
    int groups_per_wave;     // 16-row groups each wavefront walks
    const uint16_t* raw;     // non-NULL: test `normalized <= 0.9` on the raw pixels (dense rows of N) instead of reading `normalized`
    const uint32_t* minmax;
    int min_chain_exact;
    const uint32_t* only_if; // non-NULL: images whose word is 0 are skipped (fix-up launch behind the fused expand kernel)
};

// kernels_pyramid.hip
// swz: the XCD-aware workgroup -> tile mapping of the marching kernels (kernels_common.h xcd_tile, role_tile), 0 or 1; regions: the
// metric kernel's 2-D regions per XCD (xcd_region_tile) where its geometry allows, 0 or 1. A context reads both once, in create_impl
// (MUSICA_XCD_SWIZZLE, MUSICA_XCD_REGIONS), and hands them to every launch (ExpandArgs::swz, RbSdevArgs::swz likewise).
// ref != 0 (generic kernels only): the shaders' literal 25-tap accumulation order (MUSICA_FLAG_REFERENCE_ORDER)
void launch_reduce(hipStream_t st, const float* in, const LevelDesc& li, float* out, const LevelDesc& lo, int batch, bool force_generic, int tag,
                   int swz, int regions, int ref = 0);
void launch_band(hipStream_t st, const float* fine, const float* coarse, float* band, const LevelDesc& lf, const LevelDesc& lc, int batch, int ref = 0);
void launch_reduce_band_u16(hipStream_t st, const uint16_t* px, float* down, float* band, const LevelDesc& lf, const LevelDesc& lc, int batch,
                            int rows_per_wave, const uint32_t* minmax, int min_chain_exact, uint16_t* le090, int swz);
void launch_reduce_band(hipStream_t st, const float* fine, float* down, float* band, const LevelDesc& lf, const LevelDesc& lc, int batch, int rows_per_wave,
                        int swz);
void launch_lowpass(hipStream_t st, const float* coarse, float* low, const LevelDesc& lf, const LevelDesc& lc, int batch, int ref = 0);
void launch_expand(hipStream_t st, const ExpandArgs& a, int gain_mode, bool nr, int batch, bool force_generic);   // a.sdev == nullptr (GAIN_CURVE): hands over to launch_expand_sd
// reduce + band of the levels in `a`, then their expand slots, one workgroup per image (levels of side <= kTailSide)
void launch_tiny_tail(hipStream_t st, const TailArgs& a, int batch);
void launch_exp_band(hipStream_t st, const ExpandArgs& a, int gain_mode, bool nr, int batch);
// kernels_expand_sd.hip (the pyramid launches that keep a window of squares in registers)
// reduce + band of level i + 1 AND the sdev + noise-histogram pass of level i in one launch (both read what the reduce + band launch of level i wrote
// and nothing of each other). Workgroups 0 .. of grid.x take the sdev pass (sl.first = 0), the rest the reduce + band launch.
struct RbSdevArgs {
    const float* fine; float* down; float* band;   // reduce + band of level i + 1: its fine image, coarse image, band image
    int S, pitch; size_t plane; int Sc, cpitch; size_t cplane; int rows_rb;
    int rb_strips, rb_blocks, rb_first;            // that role's workgroups: rb_strips * rb_blocks from rb_first on (a multiple of 8)
    SdevRunLevel sl;                               // level i's pass: march (sl.rows > 0) or one run per workgroup; sl.sdev == nullptr: histogram only;
                                                   // sl.rows < 0 (level 0): its reduce + band launch counted the histogram, the role is the seam pass
    size_t hist_stride; int cov, swz;
    int seam_items;                                // filled in by launch_rb_sdev
};
void launch_rb_sdev(hipStream_t st, RbSdevArgs a, const LevelDesc& ls, int batch);
// launch_reduce_band_u16 that also counts level 0's noise histogram (k_reduce_band_hist) except for the two columns
// either side of every interior strip boundary: launch_hist_seam, or the sdev role of launch_rb_sdev with sl.rows < 0, counts those from
// the stored band image. rows_per_wave % 8 == 0. hist: image 0's level-0 histogram.
void launch_reduce_band_u16_hist(hipStream_t st, const uint16_t* px, float* down, float* band, const LevelDesc& lf, const LevelDesc& lc, int batch,
                                 int rows_per_wave, const uint32_t* minmax, int min_chain_exact, uint16_t* le090, int swz, uint32_t* hist,
                                 size_t hist_stride, int cov);
void launch_hist_seam(hipStream_t st, const float* band, const LevelDesc& l, uint32_t* hist, size_t hist_stride, int cov, int batch);
void launch_expand_sd(hipStream_t st, const ExpandArgs& a, bool nr, int batch);   // a.sdev == nullptr: sdev computed by the launch
// kernels_analysis.hip
void launch_clear(hipStream_t st, uint32_t* minmax, uint32_t* noise_hist, uint32_t* grad_hist, uint32_t* clahe_hist, int batch, uint32_t* grad_hist_b = nullptr, uint32_t* gzero = nullptr);
// min / max of the raw pixels (slots: [batch][kMinMaxSlots] words, ticket: [batch] words, zero at first use) and, where the pointers are
// given, the clears of src/vk_processing.cpp:2153-2162 in the same launch
constexpr int kMinMaxSlots = 4096;
void launch_minmax(hipStream_t st, const uint16_t* px, int N, uint32_t* minmax, uint32_t* slots, uint32_t* ticket, int batch,
                   uint32_t* noise_hist = nullptr, uint32_t* grad_hist = nullptr, uint32_t* grad_hist_b = nullptr, uint32_t* gzero = nullptr,
                   uint32_t* clahe_hist = nullptr);
void launch_normalize(hipStream_t st, const uint16_t* px, float* out, const LevelDesc& l0, const uint32_t* minmax, int min_chain_exact, int batch);
void launch_sqrt(hipStream_t st, const uint16_t* px, float* out, const LevelDesc& l0, int batch);
// the sdev + noise-histogram passes (fast order) of n <= kSdevRunLevelsMax levels in ONE launch of k_sdev_hist, each level in its own form
// (rows[k] > 0: the march with that many rows per wavefront, 0: one 16-row run per workgroup); sdev[k] == nullptr: histogram only; hist[k]:
// image 0's histogram of level k; hist == nullptr: the sdev images alone (marches only, sides that are multiples of 8)
void launch_sdev_hist(hipStream_t st, int n, const float* const* band, float* const* sdev, const LevelDesc* lv, uint32_t* const* hist,
                      const int* rows, size_t hist_stride, int cov, int batch, int swz);
void launch_noise_hist_only(hipStream_t st, const float* sdev, const LevelDesc& l, uint32_t* hist, size_t hist_stride, int cov, int batch);
// img_sdev.comp:10-35 with the 25 squares accumulated in the shader's order (one thread per texel; MUSICA_FLAG_REFERENCE_ORDER)
void launch_sdev_literal(hipStream_t st, const float* band, float* sdev, const LevelDesc& l, int batch);
void launch_curves_cnr(hipStream_t st, const uint32_t* hist, size_t hist_stride, musica_hist_max_point* maxpts, DevCurve* curves,
                       const musica_contrast_params* cparams, int levels, int batch, DevCurveLut* luts, const float* sdev, float* cnr,
                       const LevelDesc& l3, const uint32_t* minmax, int min_chain_exact, int* thr090, int lev0 = 0);
void launch_selftest_exact_math(hipStream_t st, unsigned long long* d_bad4);
// the RGBA plots of RENDER_HISTS (kernels_gradation.hip): out = MUSICA_HIST_RENDER_WIDTH x MUSICA_HIST_RENDER_HEIGHT packed texels
void launch_render_noise_hist(hipStream_t st, const uint32_t* hist, const musica_hist_max_point* maxpt, uint32_t* out);
void launch_render_grad_hist(hipStream_t st, const uint32_t* hist, const musica_hist_max_point* maxpt, const DevCurve* curve, uint32_t* out);
constexpr int kStatsMaxBlocks = 64;
void launch_stats(hipStream_t st, const float* cnr, const LevelDesc& l3, const uint32_t* minmax, int min_chain_exact,
                  const musica_hist_max_point* noise_max, int levels, const musica_hist_max_point* grad_max, const DevCurve* gcurve,
                  musica_stats* out, uint32_t image_id_base, uint32_t image_id_stride, int batch, double* partial);
// kernels_gradation.hip
void launch_grad_hist(hipStream_t st, const GradArgs& a, int batch);
void launch_relevant(hipStream_t st, const float* normalized, const float* cnr, float* out, const LevelDesc& l0, const LevelDesc& l3,
                     int cnrScale, int batch, const uint16_t* raw = nullptr, const int* thr090 = nullptr);
// recount (images whose a.only_if word is set, into a.hist) + tone curve in one launch; ticket: [batch][kGradTicketStride] words, zero
constexpr int kGradTicketStride = 32;
void launch_grad_recount_curve(hipStream_t st, const GradArgs& a, uint32_t* hist, musica_hist_max_point* gmax, DevCurve* curves, uint32_t* ticket, int batch);
void launch_grad_curve(hipStream_t st, uint32_t* hist, musica_hist_max_point* gmax, DevCurve* curves, int batch, const uint32_t* hist_b = nullptr, const uint32_t* gzero = nullptr);
void launch_grad_apply(hipStream_t st, const float* in, float* out, const LevelDesc& l0, const DevCurve* curves, int batch);
// crop + quantise of saveOutImage for ONE image plane: out = (S - 2 margin)^2 bytes, dense
void launch_out_pixels(hipStream_t st, const float* graded, const LevelDesc& l0, int margin, uint8_t* out);
void launch_out_bmp24(hipStream_t st, const float* graded, const LevelDesc& l0, int margin, uint32_t* out);   // the BMP file's pixel array (24 bpp, bottom-up, padded rows)
// kernels_export.hip: the same crop + quantise for `count` image planes from `graded` on (stride l0.plane) in one launch; image k's row r at
// dst + k * image_pitch + r * row_pitch (bytes), nothing else written
void launch_export_u8(hipStream_t st, const float* graded, const LevelDesc& l0, int count, uint8_t* dst, size_t row_pitch, size_t image_pitch);
// The two w x h regions a query of the study compares (musica_study.hip sim_region). a: the graded f32 plane at the region's origin
// (margin included), b: the reference slot's u8 plane at its origin.
struct SimRegion {
    const float* a;
    const uint8_t* b;
    int a_pitch, b_pitch;   // elements
    int w, h;
};
// kernels_similarity.hip: one comparison of musica_sim_compare. strips / segs / seg_rows: launch geometry (sim_geometry).
struct SimQueryDev : SimRegion {
    int strips, segs, seg_rows;
};
struct SimPart {
    double ssim;              // sum of the per-pixel SSIM over the interior the workgroup computes
    unsigned long long ssd;   // sum of squared differences over the pixels it owns
};
struct SimConsts {
    double c1, c2, cov_norm;  // (0.01 * 255)^2, (0.03 * 255)^2, 49 / 48 as harness.ssim_similarity computes them
};
constexpr int kSimMaxBlocks = 1024;   // workgroups per query (partials slots)
constexpr int kSimTile = 64;          // MUSICA_SIM_TILE: the tiles of k_displace, k_ens_stats, k_cov_add and k_cov_mean
constexpr int kSimMaxRadius = 16;     // MUSICA_SIM_MAX_RADIUS: the largest shift of k_displace and lag of k_cov_add / k_cov_mean
// The launch geometry of a strip march (k_sim, k_scales_win) over a w x h plane: strips of `cols` columns and, at most `cap`
// workgroups in all, segments of at least 32 rows so that the 6-row halo stays below 20 %.
void strip_geometry(int w, int h, int cols, int cap, int& strips, int& segs, int& seg_rows);
void sim_geometry(SimQueryDev& q);
// k_sim over `count` queries (grid.x = the largest strips * segs), then k_sim_fold; hist: count x [a 256 | b 256] u32, zeroed by the caller
void launch_sim(hipStream_t st, const SimQueryDev* d_qs, int count, int max_blocks, SimPart* part, uint32_t* hist, SimPart* out, const SimConsts& k);
// k_sim_vendor: `total` vendor values (u16 when bits == 16, else u8; dense, from an allocation's base) into `out` (u8, dense, from an
// allocation's base) as 255 - (v >> 8) or 255 - v
void launch_sim_vendor(hipStream_t st, const void* src, int bits, uint8_t* out, long long total);
// kernels_joint.hip: one query of musica_sim_joint. chunk_rows / chunks: launch geometry (joint_geometry): a workgroup counts
// chunk_rows whole region rows (at most 65535 pixels) between two flushes of its LDS table.
struct JointQueryDev : SimRegion {
    int chunk_rows, chunks;
};
constexpr int kJointMaxBlocks = 256;    // workgroups per launch, shared by its queries, but at least kJointMinBlocks per query; a
constexpr int kJointMinBlocks = 8;      // workgroup strides over the chunks beyond that
void joint_geometry(JointQueryDev& q, int count);   // count: the queries of the launch
// k_joint over `count` queries (grid.x = min(max_chunks, max(kJointMinBlocks, kJointMaxBlocks / count))); joint: count x 65536 u32 (row a, column b), zeroed by the caller
void launch_joint(hipStream_t st, const JointQueryDev* d_qs, int count, int max_chunks, uint32_t* joint);
// k_sim_remap: out[i] = lut[src[i]] over `total` bytes (both dense, from an allocation's base; the planes must not overlap)
struct RemapLut {
    uint8_t v[256];
};
void launch_sim_remap(hipStream_t st, const uint8_t* src, uint8_t* out, const RemapLut& lut, long long total);
// kernels_displace.hip: one query of musica_sim_displace. The b window grown by the radius lies inside the slot's plane (the caller
// checks). tiles_x / tiles_y: ceil(w / 64), ceil(h / 64); tile_base: where the query's tile tables start in the launch's tile-table
// buffer, in u32 elements (tile-row major, S^2 values per tile, S = 2 radius + 1).
struct DisplaceQueryDev : SimRegion {
    int tiles_x, tiles_y;
    unsigned long long tile_base;
};
// k_displace over `count` queries (grid.x = max_tiles, the largest tiles_x * tiles_y), then k_displace_fold. tile_tables: every query's
// tile tables (all written); tables: count x S^2 u64 and tiles_off: count u32, both zeroed by the caller.
void launch_displace(hipStream_t st, const DisplaceQueryDev* d_qs, int count, int max_tiles, int radius, uint32_t* tile_tables,
                     unsigned long long* tables, uint32_t* tiles_off);
// kernels_scales.hip: musica_sim_multiscale. One query of the pooling pass: its 64 x 16 tiles anchored at the region's origin, where its
// planes start in the call's scratch (bytes, 16-byte aligned: scale 0 as x | y << 8 in u16, scales >= 1 as x | y << 16 in u32, plane s
// dense (h >> s) x (w >> s)) and where its tiles' partials start.
constexpr int kScaleMaxScales = 5;    // MUSICA_SIM_MAX_SCALES
constexpr int kScalePoolW = 64, kScalePoolH = 16;
constexpr int kScaleMaxBlocks = 512;  // workgroups per job of the windowed launch (partials slots)
struct ScalePoolDev : SimRegion {
    int scales, tiles_x, tiles_y;
    unsigned long long plane_off[kScaleMaxScales];
    unsigned long long part_base;     // ScalePoolPart elements
};
struct ScalePoolPart {
    unsigned long long ssd[kScaleMaxScales];   // sum of (X_s - Y_s)^2 over the tile's cells of plane s
};
// One (query, scale) of the windowed launch: the plane (w x h texels at plane_off) and the launch geometry (scales_geometry).
struct ScaleJobDev {
    unsigned long long plane_off;
    int w, h, scale, query;
    int strips, segs, seg_rows;
};
struct ScaleWinPart {
    double ssim, cs, lum;             // sums over the windows the workgroup computes
};
struct ScaleOut {
    double ssim, cs, lum;             // sums over the job's windows
    unsigned long long ssd;           // the query's exact sum of (X_s - Y_s)^2 at the job's scale
};
struct ScaleConsts : SimConsts {
    double div1[kScaleMaxScales], div2[kScaleMaxScales];   // 49 * 4^s, 49 * 16^s
};
void scales_geometry(ScaleJobDev& q);
// k_scales_pool over `count` queries (grid.x = max_tiles, the largest tiles_x * tiles_y), k_scales_win over `jobs` jobs (grid.x =
// max_blocks, the largest strips * segs), then k_scales_fold: out[j] of job j. pool: the tiles' partials; part: jobs x kScaleMaxBlocks.
void launch_scales(hipStream_t st, const ScalePoolDev* d_qs, int count, int max_tiles, const ScaleJobDev* d_jobs, int jobs, int max_blocks,
                   uint8_t* scratch, ScalePoolPart* pool, ScaleWinPart* part, ScaleOut* out, const ScaleConsts& k);
// kernels_ensemble.hip: musica_sim_ensemble_*. The accumulators are one uint2 {S1, S2} per pixel of the cropped plane, dense rows.
// One query of k_ens_stats: s the accumulators at the a region's origin, b the reference slot's plane at the b region's origin, w x h
// pixels; tiles_x / tiles_y: ceil(w / 64), ceil(h / 64); tile_base: where the query's tile pairs start in the launch's tile table, in tiles.
struct EnsQueryDev {
    const uint2* s;
    const uint8_t* b;
    int s_pitch, b_pitch;   // elements
    int w, h;
    int tiles_x, tiles_y;
    unsigned long long tile_base;
};
constexpr int kEnsTotals = 6;    // u64 per query: sum D^2, sum V, sum D (two's complement), sum E, max |D|, max V
// k_ens_add: S1 += a, S2 += a^2 over the cropped plane for the `count` graded planes from `graded` on (stride l0.plane), one launch
void launch_ens_add(hipStream_t st, const float* graded, const LevelDesc& l0, int count, uint2* acc);
// k_ens_stats over `count` queries (grid.x = max_tiles, the largest tiles_x * tiles_y) after K realisations. tile_tables: two u64 per tile
// (all written); totals: count x kEnsTotals u64, zeroed by the caller.
void launch_ens_stats(hipStream_t st, const EnsQueryDev* d_qs, int count, int max_tiles, uint32_t K, unsigned long long* tile_tables,
                      unsigned long long* totals);
// kernels_covariance.hip: musica_sim_ensemble_track / _covariance. One tracked region: (ax, ay) + w x h of the cropped plane, its window
// grown by the radius left, right and downwards inside the plane (the caller checks); tiles_x / tiles_y: ceil(w / 64), ceil(h / 64);
// tile_base: where the region's tile tables start in the tile-table buffers, in u64 elements (tile-row major, (R + 1) (2 R + 1) per tile).
struct CovRegionDev {
    int ax, ay, w, h;
    int tiles_x, tiles_y;
    unsigned long long tile_base;
};
// k_cov_add: P(d) += sum over the tile of a(p) a(p + d) for the `count` graded planes from `graded` on (stride l0.plane), one launch over
// `regions` regions (grid.x = max_tiles, the largest tiles_x * tiles_y); tile_tables: u64, zeroed when tracking starts.
void launch_cov_add(hipStream_t st, const CovRegionDev* d_rs, int regions, int max_tiles, int radius, const float* graded, const LevelDesc& l0, int count,
                    unsigned long long* tile_tables);
// k_cov_mean after K realisations: tile_cov = K P - U per tile (all written), added into tables (regions x (R + 1) (2 R + 1) u64, zeroed by
// the caller; two's complement). ens: the ensemble's accumulators, dense rows of nw words.
void launch_cov_mean(hipStream_t st, const CovRegionDev* d_rs, int regions, int max_tiles, int radius, uint32_t K, const uint2* ens, int nw,
                     const unsigned long long* tile_tables, long long* tile_cov, unsigned long long* tables);
// kernels_alteration.hip: one alteration of musica_alter (or the draws of musica_alter_draws) over an n x n plane.
struct AlterDev {
    int kind;                  // MUSICA_ALTER_*
    int n;                     // side of the source and output planes
    int ys, xs, hh, ww;        // TRANSLATE: out[ys .. ys + hh) x [xs .. xs + ww) = src[top .., left ..], the rest the fill
    int top, left;
    int margin, crop;          // ROTATE: the crop [margin, margin + crop)^2 is rotated, the rest the fill
    int sh, sv;                // COLLIMATOR: shutters
    double mean, sigma;        // GAUSSIAN
    double factor;             // POISSON
    uint32_t key0, key1, stream;
    double m[4], off[2];       // ROTATE
};
// a region of a u16 plane and the percentile q (0 .. 100) of it to find
struct PctRegion {
    const uint16_t* src;
    int pitch, x, y, w, h;
    double q;
};
// out: the output plane (NULL: none), draws: n * n int32 of the noise kinds (NULL: none); fill: the device double of the geometric kinds
void launch_alter(hipStream_t st, const uint16_t* src, uint16_t* out, int32_t* draws, const AlterDev& a, const double* fill);
// ROTATE with margin 0, crop n and fill 0 over a u8 plane (a reference slot)
void launch_rotate_u8(hipStream_t st, const uint8_t* src, uint8_t* out, const AlterDev& a);
// np.percentile of the region into *out (device); hist: 768 u32 of scratch, zeroed by the caller
void launch_percentile(hipStream_t st, const PctRegion& g, uint32_t* hist, double* out);
// kernels_symmetry.hip: element 0 .. 7 of the square's symmetry group, np.rot90(x if element < 4 else x.T, element & 3), of a dense n x n
// plane into another (the planes must not overlap); any n >= 1
void launch_symmetry_u16(hipStream_t st, const uint16_t* src, uint16_t* out, int n, int element);
void launch_symmetry_u8(hipStream_t st, const uint8_t* src, uint8_t* out, int n, int element);
// kernels_blur.hip: harness.binomial_blur(plane, radius), the exact binomial blur with weights C(2 radius, k) and clamped borders, of a
// dense n x n plane into another (the planes must not overlap); any n >= 1, radius 1 .. kBlurMaxRadius
constexpr int kBlurMaxRadius = 8;   // MUSICA_BLUR_MAX_RADIUS
void launch_blur_u16(hipStream_t st, const uint16_t* src, uint16_t* out, int n, int radius);
void launch_blur_u8(hipStream_t st, const uint8_t* src, uint8_t* out, int n, int radius);
// kernels_codec.hip: metrics.block_codec(plane, table, (origin, origin)), the exact 8 x 8 integer block codec, of a dense n x n plane into
// another (the planes must not overlap); any n >= 1, origin 0 .. 7, every table entry 1 .. 65535 (q[v * 8 + u], v the vertical
// frequency).
struct CodecTable {
    uint16_t q[64];
};
void launch_codec_u16(hipStream_t st, const uint16_t* src, uint16_t* out, int n, int origin, const CodecTable& table);
void launch_codec_u8(hipStream_t st, const uint8_t* src, uint8_t* out, int n, int origin, const CodecTable& table);
// kernels_zoom.hip: harness.zoom(plane, (p, q)), the exact bilinear magnification by p / q about the centre, of a dense n x n plane into
// another (the planes must not overlap); any n >= 1, 1 <= q < p <= kZoomMaxP with gcd(p, q) = 1
constexpr int kZoomMaxP = 32;   // MUSICA_ZOOM_MAX_P
void launch_zoom_u16(hipStream_t st, const uint16_t* src, uint16_t* out, int n, int p, int q);
void launch_zoom_u8(hipStream_t st, const uint8_t* src, uint8_t* out, int n, int p, int q);
// kernels_scatter.hip: harness.scatter(plane, (radius, num, den)), the exact veiling glare (the plane mixed with its tent x tent blur of
// box radius `radius`, scatter fraction num / den), of a dense n x n plane into another through `plane32`, n x n u32 of scratch that the
// row launch writes and the column launch reads (none of the three may overlap); any n in 1 .. 16384, 1 <= radius <= kScatterMaxRadius,
// 1 <= num < den <= kScatterMaxDen
constexpr int kScatterMaxRadius = 127;   // MUSICA_SCATTER_MAX_RADIUS
constexpr int kScatterMaxDen = 64;       // MUSICA_SCATTER_MAX_DEN
void launch_scatter_u16(hipStream_t st, const uint16_t* src, uint16_t* out, uint32_t* plane32, int n, int radius, int num, int den);
void launch_scatter_u8(hipStream_t st, const uint8_t* src, uint8_t* out, uint32_t* plane32, int n, int radius, int num, int den);
// kernels_warp.hip: harness.warp(plane, field, (origin, origin)), the exact backward warp by a displacement field on a control grid of
// spacing kWarpGrid in units of 1 / kWarpUnit pixel, of a dense n x n plane into another (the planes must not overlap); any n >= 1,
// 0 <= origin < kWarpGrid. nodes: m x m nodes on the device, row-major, one u32 each (dx in the low half, dy in the high one, both i16
// within +-kWarpMaxShift), m >= ((n - 1 + origin) >> 6) + 2
constexpr int kWarpGrid = 64;          // MUSICA_WARP_GRID
constexpr int kWarpUnit = 256;         // MUSICA_WARP_UNIT
constexpr int kWarpMaxShift = 4096;    // MUSICA_WARP_MAX_SHIFT
void launch_warp_u16(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const uint32_t* nodes, int m, int origin);
void launch_warp_u8(hipStream_t st, const uint8_t* src, uint8_t* out, int n, const uint32_t* nodes, int m, int origin);
// kernels_details.hip: the contrast-detail relation. A detail (x, y, r, c) of a list that the caller has checked (limits, boxes inside
// the plane and pairwise disjoint), packed: a plane side is at most 16384.
constexpr int kDetailMaxRadius = 64;      // MUSICA_DETAIL_MAX_RADIUS
constexpr int kDetailMaxContrast = 512;   // MUSICA_DETAIL_MAX_CONTRAST
constexpr int kDetailMax = 1024;          // MUSICA_DETAIL_MAX
constexpr int kDetailWords = 14;          // u64 of a musica_sim_detail_result
struct PackedDetail {
    uint32_t xy;   // x | y << 16
    uint32_t rc;   // r | (c + 512) << 8
};
// harness.insert_details(src, details) of a dense n x n plane into another (the planes must not overlap); any n >= 1, `count` details
// at d_details (device)
void launch_alter_details(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const PackedDetail* d_details, int count);
// harness.detail_statistics: one workgroup per detail. a_plane: the graded f32 plane at output pixel (0, 0), b_plane: the slot's u8
// plane, pitches in elements, the details in the cropped output plane's coordinates; out: count x kDetailWords u64, all written
void launch_sim_details(hipStream_t st, const float* a_plane, int a_pitch, const uint8_t* b_plane, int b_pitch, const PackedDetail* d_details, int count,
                        unsigned long long* out);
// kernels_edges.hip: the edge-response relation. An edge (x, y, h, p, q, o, c) of a list that the caller has checked (limits, plates
// inside the plane and pairwise disjoint), packed: a plane side is at most 16384.
constexpr int kEdgeMinHalf = 8;         // MUSICA_EDGE_MIN_HALF
constexpr int kEdgeMaxHalf = 128;       // MUSICA_EDGE_MAX_HALF
constexpr int kEdgeMinQ = 4;            // MUSICA_EDGE_MIN_Q
constexpr int kEdgeMaxQ = 16;           // MUSICA_EDGE_MAX_Q
constexpr int kEdgeMaxContrast = 512;   // MUSICA_EDGE_MAX_CONTRAST
constexpr int kEdgeMax = 256;           // MUSICA_EDGE_MAX
constexpr int kEdgeBinsMax = 2048;      // MUSICA_EDGE_BINS_MAX
constexpr int kEdgeWords = 4;           // u64 of a musica_sim_edge_result
struct PackedEdge {
    uint32_t xy;      // x | y << 16
    uint32_t hpqo;    // h | p << 8 | q << 16 | o << 24
    int32_t c;        // the contrast (0 where the call does not look at it)
    uint32_t table;   // k_sim_edges: where the edge's 4 x bins words start in the flat tables
};
// harness.insert_edges(src, edges) of a dense n x n plane into another (the planes must not overlap); any n >= 1, `count` edges at
// d_edges (device)
void launch_alter_edges(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const PackedEdge* d_edges, int count);
// harness.edge_statistics: one workgroup per edge. a_plane: the graded f32 plane at output pixel (0, 0), b_plane: the slot's u8 plane,
// pitches in elements, the edges in the cropped output plane's coordinates; results: count x kEdgeWords u64, tables: every edge's
// 4 x bins u32 from its PackedEdge::table on, all written
void launch_sim_edges(hipStream_t st, const float* a_plane, int a_pitch, const uint8_t* b_plane, int b_pitch, const PackedEdge* d_edges, int count,
                      unsigned long long* results, uint32_t* tables);
// kernels_gratings.hip: the grating relation. A grating (x, y, h, ux, uy, T) of a list that the caller has checked (limits, plates
// inside the plane and pairwise disjoint), packed: a plane side is at most 16384.
constexpr int kGratingMinHalf = 8;         // MUSICA_GRATING_MIN_HALF
constexpr int kGratingMaxHalf = 128;       // MUSICA_GRATING_MAX_HALF
constexpr int kGratingMaxU = 8;            // MUSICA_GRATING_MAX_U
constexpr int kGratingMaxPeriod = 64;      // MUSICA_GRATING_MAX_PERIOD
constexpr int kGratingMaxContrast = 512;   // MUSICA_GRATING_MAX_CONTRAST
constexpr int kGratingMax = 256;           // MUSICA_GRATING_MAX
constexpr int kGratingWords = 4;           // u64 of a musica_sim_grating_result
struct PackedGrating {
    uint32_t xy;      // x | y << 16
    uint32_t htuv;    // h | T << 8 | (ux & 0xFF) << 16 | (uy & 0xFF) << 24: ux, uy as signed bytes
    uint32_t first;   // the sum of the periods before it: where its wave starts in the flat waves, and a quarter of where its table starts
};
// harness.insert_gratings(src, gratings) of a dense n x n plane into another (the planes must not overlap); any n >= 1, `count`
// gratings at d_gratings and their wave tables at d_waves, grating i's at PackedGrating::first (device)
void launch_alter_gratings(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const PackedGrating* d_gratings, const int16_t* d_waves, int count);
// harness.grating_statistics: one workgroup per grating. a_plane: the graded f32 plane at output pixel (0, 0), b_plane: the slot's u8
// plane, pitches in elements, the gratings in the cropped output plane's coordinates; results: count x kGratingWords u64, tables: every
// grating's 4 x T u32 from 4 * PackedGrating::first on, all written
void launch_sim_gratings(hipStream_t st, const float* a_plane, int a_pitch, const uint8_t* b_plane, int b_pitch, const PackedGrating* d_gratings, int count,
                         unsigned long long* results, uint32_t* tables);
// kernels_gain.hip: the detector-gain relation. harness.apply_gain(src, gx, gy) of a dense n x n plane into another (the planes must not
// overlap); any n >= 1. d_gx: the n column gains as they came (u16, a device allocation of its own), d_gy: the n row gains widened to
// u32 (the kernel fetches them on the scalar side)
constexpr int kGainOne = 4096;            // MUSICA_GAIN_ONE
constexpr int kProfileMaxQueries = 16;    // MUSICA_PROFILE_MAX_QUERIES
void launch_alter_gain(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const uint16_t* d_gx, const uint32_t* d_gy);
// One comparison of musica_sim_profiles. tiles_x / tiles_y: ceil(w / 64), ceil(h / 64); table: where its tables start in the launch's
// flat tables, in words: [w][4] then [h][4].
struct ProfileQueryDev : SimRegion {
    int tiles_x, tiles_y;
    unsigned long long table;
};
// harness.profile_statistics over `count` queries (grid.x = max_tiles, the largest tiles_x * tiles_y). tables: every query's words,
// zeroed by the caller: the tiles add their partials with u32 atomics
void launch_sim_profiles(hipStream_t st, const ProfileQueryDev* d_qs, int count, int max_tiles, uint32_t* tables);
// kernels_levels.hip: the tone-table relation. harness.apply_lut(src, lut) of a dense n x n plane into another (the planes must not
// overlap); any n >= 1. d_lut: the table's kLutEntries u16 on the device
constexpr int kLutEntries = 65536;        // a value for every u16
constexpr int kLevelMaxQueries = 4;       // MUSICA_LEVEL_MAX_QUERIES
constexpr int kLevelMinShift = 4;         // MUSICA_LEVEL_MIN_SHIFT
constexpr int kLevelMaxShift = 15;        // MUSICA_LEVEL_MAX_SHIFT
constexpr int kLevelMaxClasses = 4096;    // (65535 >> kLevelMinShift) + 1
constexpr int kLevelWords = 6;            // u64 of a class: n, sum a, sum b, sum (a - b)^2, sum a^2, sum b^2
void launch_alter_lut(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const uint16_t* d_lut);
// One comparison of musica_sim_levels. s: the source plane at side a's pixel (0, 0), s_pitch in elements; chunk_rows / chunks: launch
// geometry (level_geometry); table: where its [classes][kLevelWords] u64 start in the launch's flat tables, in words.
struct LevelQueryDev : SimRegion {
    const uint16_t* s;
    int s_pitch;
    int chunk_rows, chunks;
    unsigned long long table;
};
void level_geometry(LevelQueryDev& q, int count);   // count: the queries of the launch
// harness.level_statistics over `count` queries with the classes source >> shift (grid.x = min(max_chunks, 128 / count)). tables: every
// query's words, zeroed by the caller: the workgroups add into them with u64 atomics
void launch_sim_levels(hipStream_t st, const LevelQueryDev* d_qs, int count, int max_chunks, int shift, unsigned long long* tables);
// kernels_gradients.hip: the gradient metrics. One comparison of musica_sim_gradients: w, h >= 7 are the REGION's; the kernel tiles its
// interior, (w - 2) x (h - 2). tiles_x / tiles_y: ceil((w - 2) / 64), ceil((h - 2) / 64); tile_base: where the query's tile partials
// start in the launch's partials, in doubles; table: where its [kGradClasses][kGradWords] u64 start in the launch's flat tables, in words.
constexpr int kGradClasses = 22;          // MUSICA_GRADIENT_CLASSES: the bit lengths of B <= 1 300 500
constexpr int kGradWords = 6;             // MUSICA_GRADIENT_WORDS: n, sum A, sum B, sum dot, sum cross, neg
constexpr int kGradC = 2720;              // MUSICA_GRADIENT_C: the stabiliser of q
struct GradQueryDev : SimRegion {
    int tiles_x, tiles_y;
    unsigned long long tile_base;
    unsigned long long table;
};
// metrics.gradient_statistics over `count` queries (grid.x = max_tiles, the largest tiles_x * tiles_y), then k_gradients_fold. tables:
// every query's words, zeroed by the caller: the tiles add into them with u64 atomics; part: a double per tile (all written); out[i]: the
// sum of q over query i's interior
void launch_sim_gradients(hipStream_t st, const GradQueryDev* d_qs, int count, int max_tiles, unsigned long long* tables, double* part, double* out);
// kernels_order.hip: the local-order metric. One comparison of musica_sim_order: w, h >= 7 are the REGION's; the kernel tiles its
// interior, (w - 6) x (h - 6). tiles_x / tiles_y: ceil((w - 6) / 64), ceil((h - 6) / 64); table: where its kOrderTableWords u64 start in
// the launch's flat tables, in words.
constexpr int kOrderRings = 3;            // MUSICA_ORDER_RINGS: max(|dx|, |dy|) = 1, 2, 3 with 8, 16 and 24 neighbours
constexpr int kOrderWords = 5;            // MUSICA_ORDER_WORDS: pairs, same, reversed, flattened, split
constexpr int kOrderBins = 97;            // MUSICA_ORDER_BINS: the census distance d = 0 .. 96
constexpr int kOrderTableWords = 112;     // MUSICA_ORDER_TABLE_WORDS: [kOrderRings][kOrderWords], then [kOrderBins]
struct OrderQueryDev : SimRegion {
    int tiles_x, tiles_y;
    unsigned long long table;
};
// metrics.order_statistics over `count` queries (grid.x = max_tiles, the largest tiles_x * tiles_y). tables: every query's words,
// zeroed by the caller: the tiles add into them with u64 atomics
void launch_sim_order(hipStream_t st, const OrderQueryDev* d_qs, int count, int max_tiles, unsigned long long* tables);
// kernels_lattice.hip: the lattice sums. One comparison of musica_sim_lattice: w, h >= 2 are the REGION's; the kernel tiles its counted
// pixels, (w - 1) x (h - 1). tiles_x / tiles_y: ceil((w - 1) / 64), ceil((h - 1) / 64); groups: the persistent workgroups that share
// the tiles (lattice_groups); phase_x / phase_y: (ax + origin) mod P, (ay + origin) mod P, the class of the region's first pixel;
// table: where its P * P * kLatticeWords u64 start in the launch's flat tables, in words; part: where its `groups` partial tables of
// P * P * kLatticeWords u32 start in the launch's partials, in words.
constexpr int kLatticeWords = 8;          // MUSICA_LATTICE_WORDS: n, a, b, dd, the squared steps right of a and b, down of a and b
constexpr int kLatticeMaxPeriod = 32;     // MUSICA_LATTICE_MAX_PERIOD
constexpr int kLatticeMaxQueries = 16;    // MUSICA_LATTICE_MAX_QUERIES
constexpr int kLatticeGroupTiles = 64;    // the most tiles of a workgroup: its u32 sums hold (kernels_lattice.hip, THE 32-BIT RULE)
struct LatticeQueryDev : SimRegion {
    int tiles_x, tiles_y, groups;
    int phase_x, phase_y;
    unsigned long long table, part;
};
// The workgroups of a query of `tiles` tiles at period P: every workgroup stores a partial table of 8 P^2 words (32 KiB at P = 32), so
// the larger periods take fewer workgroups with more tiles each; never more than kLatticeGroupTiles tiles each. most > 0 (the tuning
// variable MUSICA_LATTICE_GROUPS, read at every call) lowers the number: the tables do not depend on it.
inline int lattice_groups(int tiles, int period, int most = 0) {
    const int by_period = period >= 32 ? 512 : period >= 16 ? 1024 : 4096;
    const int want = most > 0 && most < by_period ? most : by_period;
    const int least = (tiles + kLatticeGroupTiles - 1) / kLatticeGroupTiles;
    return tiles < want ? tiles : (least > want ? least : want);
}
// metrics.lattice_statistics over `count` queries (grid.x = max_groups, the largest `groups`). part: room for every query's partial
// tables; tables: every query's words, zeroed by the caller: the fold launch adds into them with u64 atomics
void launch_sim_lattice(hipStream_t st, const LatticeQueryDev* d_qs, int count, int max_groups, int period, uint32_t* part, unsigned long long* tables);
// kernels_blobs.hip: the cluster metric. One comparison of musica_sim_blobs: tiles_x / tiles_y: ceil(w / 64), ceil(h / 64); table: where
// its kBlobClasses * kBlobWords u64 start in the launch's flat tables, in words; plane: where its w * h words start in each of the
// launch's u32 planes (parent, slots, labels); tile0: the launch's tiles before its own (a tile owns kBlobTileRecords records and one
// count); cap: more than w * h, the most steps of any data-dependent loop.
constexpr int kBlobClasses = 32;          // MUSICA_BLOB_CLASSES: bit_length(n) - 1 of a component of n < 2^32 pixels
constexpr int kBlobWords = 6;             // MUSICA_BLOB_WORDS: components, pixels, sum |d|, sum d^2, box area, border
constexpr int kBlobMaxQueries = 4;        // MUSICA_BLOBS_MAX_QUERIES
constexpr int kBlobTileSlots = 256;       // records of a tile's components that touch one of its sides (at most 252)
constexpr int kBlobTileRecords = kBlobTileSlots + 1;   // ... and its largest component that touches none
constexpr int kBlobSeamThreads = 128;     // k_blobs_seam: a tile's last column and last row
struct BlobRecord {
    uint32_t first, root;       // the first pixel of the tile-local component; its component's first pixel (== first: a root)
    uint32_t n, x0, y0, x1, y1, pad;
    unsigned long long sd, sdd;
};
struct BlobBest {               // the largest component of a query; zeros where nothing changed
    uint32_t n, first, x0, y0, x1, y1;
    unsigned long long sdd;
};
struct BlobQueryDev : SimRegion {
    int tiles_x, tiles_y;
    unsigned long long table, plane, tile0;
    uint32_t cap, pad;
};
struct BlobScratch {
    uint32_t* parent;           // the union-find plane, every query's w * h words
    uint32_t* slots;            // at a record's first pixel: its index in recs; written there only
    uint32_t* labels;           // the label planes, or nullptr where none are asked for
    BlobRecord* recs;           // [tiles of the launch][kBlobTileRecords]
    uint32_t* counts;           // [tiles of the launch]: the records of a tile that are in use
    unsigned long long* best;   // [kBlobMaxQueries]: the largest key, zeroed by the caller
    BlobBest* largest;          // [kBlobMaxQueries], zeroed by the caller
    uint32_t* err;              // one word, zeroed by the caller: not zero after the launch where a loop hit its cap
};
// metrics.blob_statistics over `count` queries (grid.x = max_tiles; max_pixels: the largest w * h; records: the launch's records).
// tables: every query's words, zeroed by the caller
void launch_sim_blobs(hipStream_t st, const BlobQueryDev* d_qs, int count, int max_tiles, unsigned long long max_pixels, unsigned long long records, uint32_t threshold,
                      int connectivity, const BlobScratch& s, unsigned long long* tables);
// kernels_spectrum.hip: the spectrum metric. One comparison of musica_sim_spectrum at tile T: tiled_w / tiled_h: (w / T) T, (h / T) T,
// the region cut to whole tiles (0 where it holds none); tiles_x / tiles_y: ceil(tiled_w / 64), ceil(tiled_h / 64), the 64 x 64 BLOCKS
// the kernel walks; groups: the persistent workgroups that share the blocks (spectrum_groups; 0 where there is no block); table: where
// its T * T * kSpectrumWords words start in the launch's flat tables, in words; part: where its `groups` partial tables of as many
// words start in the launch's partials, in words.
constexpr int kSpectrumWords = 3;         // MUSICA_SPECTRUM_WORDS: sum A^2, sum B^2, sum A B
constexpr int kSpectrumMaxTile = 64;      // MUSICA_SPECTRUM_MAX_TILE
constexpr int kSpectrumMaxQueries = 4;    // MUSICA_SPECTRUM_MAX_QUERIES
struct SpectrumQueryDev : SimRegion {
    int tiles_x, tiles_y, groups;
    int tiled_w, tiled_h;
    unsigned long long table, part;
};
// The workgroups of a query of `blocks` blocks: min(blocks, want), where want is kSpectrumGroups, or `most` where 0 < most < want (the
// tuning variable MUSICA_SPECTRUM_GROUPS, read at every call): the tables do not depend on it. A workgroup's 64-bit sums hold for any
// number of blocks (kernels_spectrum.hip, THE 64-BIT RULE); the number is three workgroups of 44.6 KiB LDS a compute unit on 256 of them,
// and at T = 64, where a partial table is 96 KiB, 72 MiB of partials in all; 256 and 512 measured slower at every T.
constexpr int kSpectrumGroups = 768;
inline int spectrum_groups(int blocks, int most = 0) {
    const int want = most > 0 && most < kSpectrumGroups ? most : kSpectrumGroups;
    return blocks < want ? blocks : want;
}
// metrics.spectrum_statistics over `count` queries (grid.x = max_groups, the largest `groups`, at least 1). part: room for every query's
// partial tables; tables: every query's words, zeroed by the caller: the fold launch adds into them with u64 atomics
void launch_sim_spectrum(hipStream_t st, const SpectrumQueryDev* d_qs, int count, int max_groups, int tile, unsigned long long* part, unsigned long long* tables);
// kernels_cooccurrence.hip: the texture metric. One comparison of musica_sim_cooccurrence: tiles_x / tiles_y: its region's 64 x 64
// tiles; groups: the persistent workgroups that share the tiles of ONE distance and side (cooccurrence_groups); table: where its
// distance_count * 4 * 2 * G * G words start in the launch's flat tables, in words.
constexpr int kCooccurrenceMaxDistances = 4;   // MUSICA_COOCCURRENCE_MAX_DISTANCES
constexpr int kCooccurrenceMaxDistance = 16;   // MUSICA_COOCCURRENCE_MAX_DISTANCE
constexpr int kCooccurrenceMaxLevels = 64;     // MUSICA_COOCCURRENCE_MAX_LEVELS
constexpr int kCooccurrenceMaxQueries = 4;     // MUSICA_COOCCURRENCE_MAX_QUERIES
struct CooccurrenceQueryDev : SimRegion {
    int tiles_x, tiles_y, groups;
    unsigned long long table;
};
struct CooccurrenceDistances {
    int count;
    int d[kCooccurrenceMaxDistances];
};
// The workgroups that one distance and side of a query of `tiles` tiles get: min(tiles, want), where want is kCooccurrenceGroups, or
// `most` where 0 < most < want (the tuning variable MUSICA_COOCCURRENCE_GROUPS, read at every call): the tables do not depend on it,
// a workgroup's u32 counters hold any number of tiles (kernels_cooccurrence.hip, THE WIDTH RULE). A launch has 2 * distance_count
// times as many workgroups a query; the number is a measurement.
constexpr int kCooccurrenceGroups = 256;
inline int cooccurrence_groups(int tiles, int most = 0) {
    const int want = most > 0 && most < kCooccurrenceGroups ? most : kCooccurrenceGroups;
    return tiles < want ? tiles : want;
}
// metrics.cooccurrence_statistics over `count` queries at `levels` gray levels (grid.x = max_groups, the largest `groups`, at least 1;
// grid.y = 2 * dist.count). tables: every query's words, zeroed by the caller: the workgroups add into them with u32 atomics
void launch_sim_cooccurrence(hipStream_t st, const CooccurrenceQueryDev* d_qs, int count, int max_groups, int levels, const CooccurrenceDistances& dist, uint32_t* tables);
// kernels_granulometry.hip: the size metric. One comparison of musica_sim_granulometry: tiles_x / tiles_y: its region's 64 x 64 tiles;
// groups: the persistent workgroups that share the tiles of ONE polarity (granulometry_groups); table: where its
// (radius_count + 1) * 2 * kGranulometryWords words start in the launch's flat tables, in words.
constexpr int kGranulometryMaxRadii = 8;      // MUSICA_GRANULOMETRY_MAX_RADII
constexpr int kGranulometryMaxRadius = 16;    // MUSICA_GRANULOMETRY_MAX_RADIUS
constexpr int kGranulometryMaxQueries = 4;    // MUSICA_GRANULOMETRY_MAX_QUERIES
constexpr int kGranulometryWords = 5;         // MUSICA_GRANULOMETRY_WORDS
struct GranulometryQueryDev : SimRegion {
    int tiles_x, tiles_y, groups;
    unsigned long long table;
};
struct GranulometryRadii {
    int count;
    int r[kGranulometryMaxRadii];
};
// The workgroups that one polarity of a query of `tiles` tiles gets: min(tiles, want), where want is kGranulometryGroups, or `most`
// where 0 < most < want (the tuning variable MUSICA_GRANULOMETRY_GROUPS, read at every call): the tables do not depend on it, a
// workgroup's u64 table holds any number of tiles. A launch has twice as many workgroups a query; two fit a compute unit (LDS).
constexpr int kGranulometryGroups = 256;
inline int granulometry_groups(int tiles, int most = 0) {
    const int want = most > 0 && most < kGranulometryGroups ? most : kGranulometryGroups;
    return tiles < want ? tiles : want;
}
// metrics.granulometry_statistics over `count` queries (grid.x = max_groups, the largest `groups`, at least 1; grid.y = the two
// polarities). tables: every query's words, zeroed by the caller: the workgroups add into them with u64 atomics
void launch_sim_granulometry(hipStream_t st, const GranulometryQueryDev* d_qs, int count, int max_groups, const GranulometryRadii& radii, unsigned long long* tables);
// kernels_contours.hip: the contour metric. One comparison of musica_sim_contours: tiles_x / tiles_y: its region's 64 x 64 tiles;
// groups: the persistent workgroups that share the tiles of ONE direction (contours_groups); table: where its 2 * (radius^2 + 2) words
// start in the launch's flat tables, in words; bits: where its two bit planes (side a, then side b: h rows of row_words u64, bit x & 63
// of word x >> 6 = pixel x) start in the scratch, in words; plane: where its byte plane starts, in bytes.
constexpr int kContoursMaxRadius = 32;             // MUSICA_CONTOURS_MAX_RADIUS
constexpr int kContoursMaxQueries = 4;             // MUSICA_CONTOURS_MAX_QUERIES
constexpr uint32_t kContoursMaxThreshold = 1300500u;   // MUSICA_CONTOURS_MAX_THRESHOLD: kernels_gradients.hip's kGradMaxTerm
struct ContourQueryDev : SimRegion {
    int tiles_x, tiles_y, groups, row_words;
    unsigned long long table, bits, plane;
};
// The workgroups that one direction of a query of `tiles` tiles gets: min(tiles, want), where want is kContoursGroups, or `most`
// where 0 < most < want (the tuning variable MUSICA_CONTOURS_GROUPS, read at every call): the tables do not depend on it.
constexpr int kContoursGroups = 1024;
inline int contours_groups(int tiles, int most = 0) {
    const int want = most > 0 && most < kContoursGroups ? most : kContoursGroups;
    return tiles < want ? tiles : want;
}
// metrics.contour_statistics over `count` queries: k_contour_mask (grid.x = max_tiles, the most tiles of a query; grid.z the queries)
// writes every word of the bit planes, the byte planes where `planes` is not null, and adds the set sizes to counts[query][side]
// (zeroed by the caller); k_contour_distance (grid.x = max_groups, grid.y = the two directions) adds into the tables, zeroed by the
// caller, with u64 atomics
void launch_sim_contours(hipStream_t st, const ContourQueryDev* d_qs, int count, int max_tiles, int max_groups, uint32_t threshold, int radius,
                         unsigned long long* bits, unsigned long long* counts, uint8_t* planes, unsigned long long* tables);
// kernels_minkowski.hip: the shape metric. One comparison of musica_sim_minkowski: tiles_x / tiles_y: its region's 64 x 64 tiles;
// groups: the persistent workgroups that share the tiles of ONE side (minkowski_groups); table: where its
// kMinkowskiSides * kMinkowskiKinds * 256 words start in the launch's flat tables, in words.
constexpr int kMinkowskiMaxQueries = 4;   // MUSICA_MINKOWSKI_MAX_QUERIES
constexpr int kMinkowskiKinds = 8;        // MUSICA_MINKOWSKI_KINDS
constexpr int kMinkowskiSides = 3;        // MUSICA_MINKOWSKI_SIDES
struct MinkowskiQueryDev : SimRegion {
    int tiles_x, tiles_y, groups;
    unsigned long long table;
};
// The workgroups that one side of a query of `tiles` tiles gets: min(tiles, want), where want is kMinkowskiGroups, or `most` where
// 0 < most < want (the tuning variable MUSICA_MINKOWSKI_GROUPS, read at every call): the tables do not depend on it, a workgroup's
// u32 counters hold any number of tiles (kernels_minkowski.hip, THE WIDTH RULE). A launch has three times as many workgroups a query.
constexpr int kMinkowskiGroups = 256;
inline int minkowski_groups(int tiles, int most = 0) {
    const int want = most > 0 && most < kMinkowskiGroups ? most : kMinkowskiGroups;
    return tiles < want ? tiles : want;
}
// metrics.minkowski_statistics over `count` queries (grid.x = max_groups, the largest `groups`, at least 1; grid.y = the three sides).
// tables: every query's words, zeroed by the caller: the workgroups add into them with u32 atomics
void launch_sim_minkowski(hipStream_t st, const MinkowskiQueryDev* d_qs, int count, int max_groups, uint32_t* tables);
// kernels_reach.hip: the reach metric. The class of a pixel of the n x n input plane is the first radius of an ascending list whose
// Chebyshev box around the pixel holds a changed input pixel (metrics.reach_classes); a comparison's exact sums are kept apart by it.
constexpr int kReachMaxRadii = 32;        // MUSICA_REACH_MAX_RADII
constexpr int kReachMaxRadius = 16383;    // MUSICA_REACH_MAX_RADIUS
constexpr int kReachMaxQueries = 16;      // MUSICA_REACH_MAX_QUERIES
constexpr int kReachWords = 6;            // MUSICA_REACH_WORDS: n, changed, sum a, sum b, sum (a - b)^2, max |a - b|
// The summed-area table of source != altered (two dense n x n u16 planes, any alignment of 2 bytes, any n in 1 .. 16384) into `sat`,
// n x n u32: sat[y * n + x] = the changed pixels of rows 0 .. y, columns 0 .. x; sat[n * n - 1] is their number. Two launches: the
// rows' inclusive prefix counts, then the running sums down the columns, in place.
void launch_reach_table(hipStream_t st, const uint16_t* source, const uint16_t* altered, uint32_t* sat, int n);
// One comparison of musica_sim_reach. sx, sy: where a-side pixel (0, 0) lies in the n x n input plane (the margin added by the caller);
// tiles_x / tiles_y: ceil(w / 64), ceil(h / 64); table: where its [radii + 1][kReachWords] u64 start in the launch's flat tables, in words.
struct ReachQueryDev : SimRegion {
    int sx, sy;
    int tiles_x, tiles_y;
    unsigned long long table;
};
// metrics.reach_statistics over `count` queries (grid.x = max_tiles, the largest tiles_x * tiles_y) with the classes of the K radii at
// d_radii (device, ascending from 0). tables: every query's words, zeroed by the caller: the tiles add into them with u64 atomics
void launch_sim_reach(hipStream_t st, const ReachQueryDev* d_qs, int count, int max_tiles, const uint32_t* sat, int n, const uint32_t* d_radii, int K,
                      unsigned long long* tables);
// metrics.reach_classes cropped by `margin`: the (n - 2 margin)^2 classes as bytes into dst (device), nothing else written
void launch_reach_classes(hipStream_t st, const uint32_t* sat, int n, int margin, const uint32_t* d_radii, int K, uint8_t* dst);
// kernels_points.hip: the point-response relation. A point (x, y, R, s, c, group) of a list that the caller has checked (limits, one R,
// windows inside the plane and pairwise disjoint), packed: a plane side is at most 16384.
constexpr int kPointMinRadius = 4;           // MUSICA_POINT_MIN_RADIUS
constexpr int kPointMaxRadius = 32;          // MUSICA_POINT_MAX_RADIUS
constexpr int kPointMaxSize = 3;             // MUSICA_POINT_MAX_SIZE
constexpr int kPointMinContrast = -64512;    // MUSICA_POINT_MIN_CONTRAST
constexpr int kPointMaxContrast = 1024;      // MUSICA_POINT_MAX_CONTRAST
constexpr int kPointMaxGroups = 16;          // MUSICA_POINT_MAX_GROUPS
constexpr int kPointMax = 4096;              // MUSICA_POINT_MAX
constexpr int kPointWords = 6;               // u64 of a musica_sim_point_result
constexpr int kPointChunk = 64;              // points of one workgroup of k_sim_points
constexpr int kPointMaxChunks = kPointMax / kPointChunk + kPointMaxGroups;   // every group may end on a ragged chunk
constexpr int kPointTableWords = kPointMaxGroups * 3 * (2 * kPointMaxRadius + 1) * (2 * kPointMaxRadius + 1);   // the largest tables
constexpr int kPointPlanWords = kPointMax + 3 * kPointMaxChunks;                                                  // the largest plan
struct PackedPoint {
    uint32_t xy;     // x | y << 16
    uint32_t rsgc;   // R | s << 6 | group << 8 | (c - kPointMinContrast) << 12
};
constexpr int kPointTileRows = 16384 / 64;   // the tile rows of the largest plane (musica_create): point_rows' entries behind a list
// Orders a packed list by y and appends one {first, count} entry per tile row of a plane of side n: what launch_alter_points takes
void point_rows(std::vector<PackedPoint>& packed, int n);
// harness.insert_points(src, points) of a dense n x n plane into another (the planes must not overlap); any n >= 1, `count` points at
// d_points (device) as point_rows left them, the tile rows' entries behind them
void launch_alter_points(hipStream_t st, const uint16_t* src, uint16_t* out, int n, const PackedPoint* d_points, int count);
// How launch_sim_points walks a list (host): the indices ordered by group, then the chunks; returns the chunks (kernels_points.hip)
int point_plan(const PackedPoint* points, int count, std::vector<uint32_t>& plan);
// harness.point_statistics: one workgroup per chunk of `plan` (point_plan's words on the host, copied to d_plan, kPointPlanWords u32 on
// the device, on the stream: `plan` must live until the stream has been waited for). a_plane: the graded f32 plane at output pixel
// (0, 0), b_plane: the slot's u8 plane, pitches in elements, the points in the cropped output plane's coordinates, all of half-side
// `radius`; results: count x kPointWords u64, all written; tables: [groups][3][(2 radius + 1)^2] u32, zeroed here on the stream
void launch_sim_points(hipStream_t st, const float* a_plane, int a_pitch, const uint8_t* b_plane, int b_pitch, const PackedPoint* d_points, int count, int radius,
                       int groups, const uint32_t* plan, int chunks, uint32_t* d_plan, unsigned long long* results, uint32_t* tables);
// kernels_observer.hip: the model-observer relation. A view (x, y, bank) of a list that the caller has checked (limits, windows inside
// the plane; they may overlap), with what the kernel needs of its bank.
constexpr int kObserverMaxViews = 1024;      // MUSICA_OBSERVER_MAX_VIEWS
constexpr int kObserverMaxBanks = 8;         // MUSICA_OBSERVER_MAX_BANKS
constexpr int kObserverMaxChannels = 16;     // MUSICA_OBSERVER_MAX_CHANNELS
constexpr int kObserverMaxHalf = 66;         // MUSICA_OBSERVER_MAX_HALF
constexpr int kObserverBlock = 8;            // channels of one workgroup of k_observer
struct PackedView {
    int32_t x, y;        // the centre
    uint32_t half;       // of its bank
    uint32_t channels;   // of its bank
    uint32_t weights;    // where its bank's words start in the call's packed weights
    uint32_t table;      // where its 2 x channels int32 start in the flat tables, in words
};
// Appends a bank's weights[channels][S][S] (S = 2 half + 1) to `words` as k_observer reads them (host): [channels][S][ceil(S / 4)]
// words of four weights each, biased to u8 (w + 128), the pad bytes of a row's last word 0
void observer_pack(const int8_t* weights, int half, int channels, std::vector<uint32_t>& words);
// metrics.channel_responses: one workgroup per view and block of kObserverBlock channels (max_channels: the largest count of the
// call's banks). a_plane: the graded f32 plane at output pixel (0, 0), b_plane: the slot's u8 plane, pitches in elements, the views in
// the cropped output plane's coordinates; tables: every view's 2 x channels int32 from its PackedView::table on, sums: count x 2 u32
// (the window's plain sums of a and b), all written
void launch_sim_observer(hipStream_t st, const float* a_plane, int a_pitch, const uint8_t* b_plane, int b_pitch, const PackedView* d_views, int count,
                         int max_channels, const uint32_t* d_weights, int32_t* tables, uint32_t* sums);
// kernels_bench.hip (measurement aid)
void launch_copy41(hipStream_t st, const float* in, float* out, int side);
// kernels_clahe.hip
void launch_clahe(hipStream_t st, const float* img, const float* relevant, float* out, const LevelDesc& l0, uint32_t* hist, musica_point* pts, int batch,
                  const uint16_t* raw = nullptr, const int* thr090 = nullptr, const float* cnr = nullptr, const LevelDesc* l3 = nullptr, int cnrScale = 0,
                  bool hist_done = false /* the histogram is already in `hist` (counted by the level-0 expand launch) */,
                  bool with_apply = true /* false: histogram + curves only, launch_grad_clahe_apply follows */);
// K21 + K24 in one pass (l0.S % 4 == 0): out_graded = tone curve of `curves`, out_clahe = CLAHE blend of `pts`
void launch_grad_clahe_apply(hipStream_t st, const float* img, float* out_clahe, float* out_graded, const LevelDesc& l0, const musica_point* pts,
                             const DevCurve* curves, int batch);

}  // namespace musica
