// curve_lut_host.cpp — the contrast curve's bucket table on the CPU: csrc/curve_lut.h (the source the kernels build and read the table
// with) against a literal getY() scan (contrast_curve_apply.comp:27-36), for every noise mode maxBin = 0 .. 2048 and the contrast
// parameters given on the command line (one lowContrastFactor per argument).
//
// For each curve: the table must exist (ok) exactly when maxBin >= 1, and lookup must equal scan bit for bit at every critical point:
// each abscissa and its +-1 and +-2 ulp neighbours, each bucket's first bit pattern and the pattern just below it, +-0, the smallest
// denormal, negatives, 1, the values around 2, +inf and NaNs. Between two neighbouring critical points both functions pick the same
// segment and evaluate the same expression, so this is a complete check.
// Prints one line "ok curves=<n> checks=<n>" and exits 0, or the first mismatches and exits 1.   (tests/test_curve_lut_host.py)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "curve_lut.h"

using namespace musica;

struct F4 { float x, y, z, w; };

// getY(): the shader's scan, the entry behind the curve reading as 0
static float scan(const float* x, const float* y, int count, float s) {
    for (int i = 0; i < count; i++) {
        const float xi = x[i];
        if (xi == s) return y[i];
        const float xn = (i + 1 < count) ? x[i + 1] : 0.0f;
        const float yn = (i + 1 < count) ? y[i + 1] : 0.0f;
        if (xi <= s && xn >= s) {
            const float m = (yn - y[i]) / (xn - xi);
            return m * (s - xi) + y[i];
        }
    }
    return 0.0f;
}

static bool same(float a, float b) { return musica_float_bits(a) == musica_float_bits(b) || (a != a && b != b); }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s low [low ...]\n", argv[0]); return 2; }
    std::vector<F4> bucket(kLutCap);
    F4 seg[kLutPoints + 1];
    std::vector<int32_t> pts;
    unsigned long long checks = 0, curves = 0, bad = 0;
    int max_entries = 0, max_inside = 0;
    for (int a = 1; a < argc; a++) {
        const float low = strtof(argv[a], nullptr);
        for (uint32_t maxBin = 0; maxBin <= 2048; maxBin++) {
            float x[kLutPoints], y[kLutPoints];
            for (int i = 0; i < kLutPoints; i++) musica_contrast_point(maxBin, low, i, x[i], y[i]);
            // the builder of k_curves_cnr (noise_curves_block)
            bool mono = x[0] == x[0];
            for (int i = 0; i + 1 < kLutPoints; i++) mono = mono && x[i] <= x[i + 1];
            const int base = musica_lut_base(x);
            const int n = (mono && x[0] == 0.0f) ? musica_lut_entries(base) : 0;
            int ok = n > 0;
            int slot[kLutPoints + 3];
            for (int i = 0; i < kLutPoints + 3; i++) slot[i] = i < kLutPoints ? musica_lut_slot(x[i], base) : kLutSlotSentinel;
            for (int k = 0; k < n; k++) {
                const int inside = musica_lut_entry(x, slot, kLutPoints, k, bucket[k]);
                if (inside > 2) ok = 0;
                if (inside > max_inside) max_inside = inside;
            }
            for (int j = 0; j <= kLutPoints; j++) musica_lut_segment(x, y, kLutPoints, j, seg[j]);
            if (n > max_entries) max_entries = n;
            curves++;
            if (ok != (maxBin >= 1 ? 1 : 0)) {
                if (bad++ < 10) printf("low %g maxBin %u: ok = %d (base %d, %d entries)\n", low, maxBin, ok, base, n);
                continue;
            }
            if (!ok) continue;
            pts.clear();
            for (int i = 0; i < kLutPoints; i++)
                for (int d = -2; d <= 2; d++) pts.push_back(musica_float_bits(x[i]) + d);   // x[0] = +0: -1, -2 are NaN patterns with the sign set
            for (int key = base - 1; key <= kLutKeyTop + 1; key++) {
                pts.push_back((int32_t)((uint32_t)key << kLutShift));
                pts.push_back((int32_t)((uint32_t)key << kLutShift) - 1);
            }
            const uint32_t fixed[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x00800000u, 0xBF800000u, 0xFF800000u, 0xFF7FFFFFu,
                                      0x3F800000u, 0x3F7FFFFFu, 0x3F800001u, 0x3FFFFFFFu, 0x40000000u, 0x40000001u, 0x7F7FFFFFu, 0x7F800000u,
                                      0x7F800001u, 0x7FC00000u, 0x7FFFFFFFu, 0xFFC00000u, 0xFF800001u};
            for (uint32_t u : fixed) pts.push_back((int32_t)u);
            for (int32_t u : pts) {
                const float s = musica_bits_float(u);
                const float got = musica_lut_eval(bucket.data(), seg, base, s), want = scan(x, y, kLutPoints, s);
                checks++;
                if (!same(got, want) && bad++ < 10)
                    printf("low %g maxBin %u s = %a (0x%08x): table %a, scan %a\n", low, maxBin, s, (unsigned)u, got, want);
            }
        }
    }
    if (bad) { printf("FAILED: %llu mismatches\n", bad); return 1; }
    printf("ok curves=%llu checks=%llu max_entries=%d max_inside=%d\n", curves, checks, max_entries, max_inside);
    return 0;
}
