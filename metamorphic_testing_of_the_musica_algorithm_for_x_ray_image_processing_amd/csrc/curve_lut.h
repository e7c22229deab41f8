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

}  // namespace musica
