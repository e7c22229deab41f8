// musica_device.h — device-side conventions shared by the kernel files and the host pipeline.
//
// Layout in HBM (one musica_ctx, batch B):
//   every f32 image of pyramid level i is stored as B planes of S_i rows with a row pitch
//   (in floats) rounded up to a multiple of 4, so every row starts 16-byte aligned and every
//   16-byte vector access inside [0, pitch) is in bounds; plane stride = pitch * S_i.
//   The raw input is dense uint16 (pitch N), exactly what the ABI hands over.
//
// Arithmetic contract (must match oracle/musica_oracle.c, MUSICA_ORDER_FAST, bit for bit):
//   IEEE binary32, no FMA contraction (this directory is compiled with -ffp-contract=off),
//   correctly rounded division and sqrt (hipcc default), left-to-right 5-tap chains that start
//   from the first product, vertical pass before horizontal pass.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/musica.h"
#include "curve_lut.h"

namespace musica {

// img_smooth.comp:23-30 — glslang folds the constant array in double and narrows once.
__device__ constexpr float W0 = 0.1f, W1 = 0.25f, W2 = 0.3f, W3 = 0.25f, W4 = 0.1f;

constexpr int kLaneCols = 8;                    // fine columns owned by one lane in the streaming kernels
constexpr int kStripCols = 64 * kLaneCols;      // fine columns covered by one 64-lane wavefront
constexpr int kWavesPerBlock = 4;
constexpr int kBlockThreads = 64 * kWavesPerBlock;

constexpr float kMaxNoiseValue = 0.1f;          // noise_hist.comp:7
constexpr float kMaxCnrValue = 256.0f;          // img_cnr.comp:6
constexpr int kHistArea = 16;                   // noise_hist.comp:5
constexpr int kMinMaxStride = 32;                // uint32 words per image in the min/max scratch (128 B)
constexpr int kMaxWord = 16;                     // the max lives one 64-byte line after the min
constexpr int kCurveCap = 64;                   // >= 33 (contrast) and 22 (gradation) points + 1 guard

// A polyline (T3 / T5 of the reference) in structure-of-arrays form plus the per-segment
// slope (p2.y - p1.y) / (p2.x - p1.x) the shaders recompute per pixel (contrast_curve_apply.comp:22-25).
// `monotone` = 1 when x[] is non-decreasing and NaN-free, which makes the shaders' first-match
// linear search equal to a binary search (see curve_eval in kernels_common.h).
struct DevCurve {
    float x[kCurveCap];
    float y[kCurveCap];
    float m[kCurveCap];
    uint32_t count;
    uint32_t monotone;
    float t0, ta, t1;       // gradation window (unused for contrast curves)
    uint32_t pad;
};

// Exact accelerator for getY() on a 33-point contrast curve (levels 0..2): j = #{x[i] < s} from ONE 16-byte table read
// and two compares, then the segment (x[j-1], y[j-1], slope[j-1]) from a second 16-byte read — no branches.
// One table keyed on the float's bit pattern (curve_lut.h has the functions, shared with the host test):
//   key(s) = bits(min(s, 2)) >> 17 (arithmetic): 64 log-spaced buckets per octave; NaN, +inf and everything above 2 take the key of
//            2.0 — above x[32] = 1, where getY() matches no interval —, a set sign bit a negative key;
//   entry k (0 .. n - 1) stands for key base + k, entry 0 also for every key below (s = +-0, negative s, positive s below the
//            bucket of x[1]: it holds x[0] = 0 alone); base = key(x[1]) - 1, n = key(2.0) - base + 1 <= kLutCap;
//   an entry stores how many abscissae lie in lower entries (jlo) and the at most two inside it (xa <= xb, +inf when absent):
//   #{x[i] < s} = jlo + (xa < s) + (xb < s).
// Membership is decided by the same function of the value when the table is built and when it is read, and that function is
// monotone (the bit pattern of a non-negative float grows with its value; the minimum, the shift and the clamp at base keep that),
// so the count is exact: an abscissa in a lower entry is < s, one in a higher entry is > s ("Exactness notes"). The
// builder verifies that the curve is monotone with 33 points, that x[0] == 0 < x[1], that the table fits kLutCap and that no entry
// holds three abscissae; otherwise (e.g. maxBin == 0) ok = 0 and the level takes the literal scan. The abscissae depend on the
// noise mode alone: every maxBin 1 .. 2048 gets a table (tests/test_curve_lut_host.py).
struct DevCurveLut {
    int32_t base;
    uint32_t ok;
    uint32_t n;          // entries in use
    uint32_t pad0;
    float4 bucket[kLutCap];                     // {16 * jlo (integer bits: byte offset of seg[jlo]), xa, xb, unused}
    float4 seg[kLutPoints + 1];                 // seg[j] = {x[j-1], y[j-1], slope[j-1], 0}; seg[0] = {x[0], y[0], 0, 0}; seg[33] = 0
};

struct LevelDesc {
    int S;          // side
    int pitch;      // row pitch in floats (multiple of 4)
    size_t plane;   // floats per image plane = pitch * S
};

// the levels of one k_sdev_hist launch (kernels_analysis.hip): workgroups first .. of grid.x take level k's pass (sdev_parts.h
// sdev_level_block); the sdev role of k_rb_sdev (kernels_expand_sd.hip) is one such level
constexpr int kSdevRunLevelsMax = 4;
struct SdevRunLevel {
    const float* band;
    float* sdev;      // nullptr: histogram only
    uint32_t* hist;   // image 0's histogram of this level (not read by a launch without histogram)
    size_t plane;
    int S, pitch, strips, first;
    int rows;         // rows per wavefront of a level that marches, 0 for a level that takes one 16-row run per workgroup
    int blocks;       // workgroups per strip
};
struct SdevRunLevels {
    SdevRunLevel l[kSdevRunLevelsMax];
    int n;
    int swz;          // XCD-aware workgroup -> tile mapping inside a level (kernels_common.h role_tile)
};

// the levels of one k_tiny_tail launch (kernels_pyramid.hip): level T + k reads `fine`, writes its reduced image `down`, its
// band-pass image and its reconstruction; Sl / lpitch / lplane: the geometry of the last level's `down` (the coarsest image)
constexpr int kTailMax = 8;
constexpr int kTailSide = 32;   // finest level the tail takes
struct TailLevel {
    const float* fine;
    float* down;
    float* band;
    float* recon;
    size_t plane;
    int S, pitch;
    float high;   // highContrastFactor of the level (GAIN_CONST)
};
struct TailArgs {
    TailLevel l[kTailMax];
    size_t lplane;
    int n, Sl, lpitch, ref;
};

static inline int round_up4(int v) { return (v + 3) & ~3; }

}  // namespace musica
