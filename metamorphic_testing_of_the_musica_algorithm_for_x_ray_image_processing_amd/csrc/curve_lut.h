// curve_lut.h — the contrast polyline's points, the bucket table that accelerates getY() on it and the lookup through that table, in
// one source for the kernels (k_curves_cnr builds the table, k_expand_fast reads it) and for the host (tests/curve_lut_host.cpp checks
// lookup against literal scan at every critical point of every noise mode). No HIP types: the 16-byte entries are any struct with
// float members x, y, z, w.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "exact_math.h"   // MUSICA_HD

namespace musica {

constexpr int kLutPoints = 33;      // 3 x generateCurve(i <= 10), contrast_curve_generate.comp:72-86
// The bucket of a value is a function of its BIT PATTERN: (bits(min(s, 2)) >> kLutShift), i.e. 2^(23 - kLutShift) = 64 log-spaced
// buckets per octave. For non-negative floats the pattern is monotone in the value, the shift keeps that, and min(s, 2) sends NaN (musica_lut_clamp),
// +inf and everything above 2 to the key of 2.0; a set sign bit (-0 included) gives a negative key.
// Table entry k (k = 0 .. n - 1) stands for key base + k, entry 0 for every key <= base as well; the last one is the key of 2.0.
constexpr int kLutShift = 17;
constexpr int kLutKeyTop = 0x40000000 >> kLutShift;   // key of 2.0f
// base = key(x[1]) - 1 per curve. The abscissae depend on the noise mode p = maxBin / 2048 * 0.1 alone; over maxBin 1 .. 2048 the keys
// from the smallest positive abscissa (maxBin = 1) to 2.0 span 1155 buckets and none holds more than two abscissae (with a shift of 18
// seven noise modes would). A curve that needs more entries, or three abscissae in one bucket, takes the literal scan (ok = 0).
constexpr int kLutCap = 1160;

MUSICA_HD int32_t musica_float_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_int(f);
#else
    int32_t i;
    memcpy(&i, &f, sizeof i);
    return i;
#endif
}
MUSICA_HD float musica_bits_float(int32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __int_as_float(i);
#else
    float f;
    memcpy(&f, &i, sizeof f);
    return f;
#endif
}
// min(s, 2) with every NaN becoming 2, spelled as the select it is: fminf() is the same for quiet NaNs, but what it returns for a
// signalling one differs between C libraries and the GPU's minimum instruction.
MUSICA_HD float musica_lut_clamp(float s) { return s < 2.0f ? s : 2.0f; }
// The key of a value already clamped; arithmetic shift.
MUSICA_HD int musica_lut_key_clamped(float sf) { return musica_float_bits(sf) >> kLutShift; }
MUSICA_HD int musica_lut_key(float s) { return musica_lut_key_clamped(musica_lut_clamp(s)); }
// Table index of a key: the one expression the builder and the lookup share.
MUSICA_HD int musica_lut_index(int key, int base) { return (key > base ? key : base) - base; }

// interpolate() of contrast_curve_generate.comp:28-31
MUSICA_HD float interpolate(float from, float to, float percent) {
    float difference = to - from;
    return from + (difference * percent);
}
// One point of generateCurve() (contrast_curve_generate.comp:39-54): step k of the quadratic Bezier (s, m, e), t = k / 10.
MUSICA_HD void bezier_point(float sx, float sy, float mx, float my, float ex, float ey, uint32_t k, float& x, float& y) {
    const float t = (float)k / 10.0f;
    const float xa = interpolate(sx, mx, t);
    const float ya = interpolate(sy, my, t);
    const float xb = interpolate(mx, ex, t);
    const float yb = interpolate(my, ey, t);
    x = interpolate(xa, xb, t);
    y = interpolate(ya, yb, t);
}
// Point i (0 .. 32) of the 33-point contrast curve of a level with lowContrastFactor `low` whose noise histogram peaks at maxBin
// (contrast_curve_generate.comp:71-86; 2048 noise bins over [0, 0.1]: noise_hist.comp:6-7).
MUSICA_HD void musica_contrast_point(uint32_t maxBin, float low, int i, float& x, float& y) {
    const float p = (float)maxBin * (1.0f / 2048.0f) * 0.1f;  // :71
    const int seg = i / 11;
    const uint32_t k = (uint32_t)(i - seg * 11);
    if (seg == 0) bezier_point(0.0f, 1.0f, p * 4.0f / 5.0f, low, p, low, k, x, y);                               // :72-76
    else if (seg == 1) bezier_point(p, low, p * 6.0f / 5.0f, low, p * 7.0f / 5.0f, low * 4.0f / 5.0f, k, x, y);   // :77-81
    else bezier_point(p * 7.0f / 5.0f, low * 4.0f / 5.0f, p * 2.0f, 1.0f, 1.0f, 1.0f, k, x, y);                   // :82-86
}

// base of a curve's table and the number of entries it uses (0: the curve cannot have a table).
MUSICA_HD int musica_lut_base(const float* x) { return musica_lut_key(x[1]) - 1; }
MUSICA_HD int musica_lut_entries(int base) {
    const int n = kLutKeyTop - base + 1;
    return (base >= 0 && n <= kLutCap) ? n : 0;
}
// Table index of abscissa x (the builder publishes b[i] = musica_lut_slot(x[i], base) for i < count and three sentinels behind them).
MUSICA_HD int musica_lut_slot(float x, int base) { return musica_lut_index(musica_lut_key(x), base); }
constexpr int kLutSlotSentinel = 0x7FFFFFFF;
// Entry k of the table over the abscissae x[0 .. count) with slots b[0 .. count) — non-decreasing, because x is (the builder checks) and
// the slot is a monotone function of the value — and b[count .. count + 2] = kLutSlotSentinel: {16 * jlo as integer bits (the byte offset
// of seg[jlo]), xa, xb, 0} with jlo = how many abscissae fall into lower entries (a 6-step search: count <= 63) and xa <= xb the at most
// two inside this one (+inf when absent). Returns how many fell inside, 3 standing for three or more.
template <class F4>
MUSICA_HD int musica_lut_entry(const float* x, const int* b, int count, int k, F4& e) {
    int jlo = 0;
    for (int step = 32; step >= 1; step >>= 1) {
        const int probe = jlo + step;
        if (probe <= count && b[probe - 1] < k) jlo = probe;
    }
    const bool ia = b[jlo] == k, ib = b[jlo + 1] == k, ic = b[jlo + 2] == k;
    e.x = musica_bits_float(jlo * 16);
    e.y = ia ? x[jlo] : (float)INFINITY;
    e.z = ib ? x[jlo + 1] : (float)INFINITY;
    e.w = 0.0f;
    return (ia ? 1 : 0) + (ib ? 1 : 0) + (ic ? 1 : 0);
}
// seg[j] = {x[j-1], y[j-1], slope[j-1], 0} for j = 1 .. count - 1, seg[0] = {x[0], y[0], 0, 0}, zeros from count on: the slopes are
// linearFunction()'s (contrast_curve_apply.comp:22-25).
template <class F4>
MUSICA_HD void musica_lut_segment(const float* x, const float* y, int count, int j, F4& sg) {
    sg.x = sg.y = sg.z = sg.w = 0.0f;
    if (j == 0) { sg.x = x[0]; sg.y = y[0]; }
    else if (j < count) { sg.x = x[j - 1]; sg.y = y[j - 1]; sg.z = (y[j] - y[j - 1]) / (x[j] - x[j - 1]); }
}
// getY() through the table (the proof is with DevCurveLut, musica_device.h): one 16-byte entry read, two compares, one 16-byte segment read.
// The index costs a minimum, a shift, a maximum and the address arithmetic.
template <class F4>
MUSICA_HD float musica_lut_eval(const F4* bucket, const F4* seg, int base, float s) {
    const float sf = musica_lut_clamp(s);
    const int idx = musica_lut_index(musica_lut_key_clamped(sf), base);
    const F4 e = *reinterpret_cast<const F4*>(reinterpret_cast<const char*>(bucket) + (uint32_t)idx * 16u);
    // e.x holds 16 * jlo as an integer (the byte offset of seg[jlo]); each abscissa of the bucket below sf moves one entry on
    const int joff = musica_float_bits(e.x) + (e.y < sf ? 16 : 0) + (e.z < sf ? 16 : 0);
    const F4 g = *reinterpret_cast<const F4*>(reinterpret_cast<const char*>(seg) + joff);
    const float r = g.z * (sf - g.x) + g.y;
    return sf < 0.0f ? 0.0f : r;
}
// musica_lut_eval for an argument whose sign bit is clear unless it is a NaN: +0, a positive number, +inf, or any NaN. That is what
// musica_rms25_8 (exact_math.h) leaves, the sdev the expand launches compute in registers: its sums are sums of squares, each +0, positive,
// +inf or NaN, so a sum is never negative and never -0; musica_sqrt_core of +0 is +0 and of a positive number is sqrtf's positive value
// (checked over all patterns on the GPU); sqrtf(x / 25.0f) of such a sum is +0, positive, +inf or NaN. A stored sdev image can hold what
// a caller injected, so the launches that read one keep musica_lut_eval. With such an argument, bit for bit the same value in fewer
// instructions:
//   * non-negative floats order like their patterns taken as unsigned integers, 2.0f is 0x40000000, and every NaN pattern (either sign)
//     is above 0x7F800000: musica_lut_clamp(s) is the pattern's unsigned minimum with 0x40000000 — one instruction, no NaN quieting;
//   * the key is then 0 .. kLutKeyTop, and base >= 0 wherever a table exists (musica_lut_entries): max(key, base) - base is key - base
//     saturating at 0, an index 0 .. kLutKeyTop - base = n - 1 as before;
//   * sf >= +0, so the `sf < 0 ? 0 : r` select never takes its first arm.
MUSICA_HD uint32_t musica_usub_sat(uint32_t a, uint32_t b) { return a > b ? a - b : 0u; }   // one v_sub_u32 with the clamp bit
template <class F4>
MUSICA_HD float musica_lut_eval_nonneg(const F4* bucket, const F4* seg, int base, float s) {
    const uint32_t u = (uint32_t)musica_float_bits(s);
    const uint32_t uf = u < 0x40000000u ? u : 0x40000000u;
    const float sf = musica_bits_float((int32_t)uf);
    const uint32_t idx = musica_usub_sat(uf >> kLutShift, (uint32_t)base);
    const F4 e = *reinterpret_cast<const F4*>(reinterpret_cast<const char*>(bucket) + idx * 16u);
    const int joff = musica_float_bits(e.x) + (e.y < sf ? 16 : 0) + (e.z < sf ? 16 : 0);
    const F4 g = *reinterpret_cast<const F4*>(reinterpret_cast<const char*>(seg) + joff);
    return g.z * (sf - g.x) + g.y;
}

}  // namespace musica
