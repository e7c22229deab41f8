// lut_nonneg_host.cpp — csrc/curve_lut.h's lookup for arguments that cannot be negative (musica_lut_eval_nonneg, what the expand launches
// that compute sdev in registers call) against the general lookup (musica_lut_eval), on the CPU, for every noise mode maxBin = 1 .. 2048
// and the lowContrastFactors given on the command line.
//
// The domain is what musica_rms25_8 can return: every pattern with the sign bit clear (+0, denormals, numbers, +inf, NaNs) and every NaN
// with the sign bit set. On it both functions must agree bit for bit. Probed per curve: each abscissa and its +-1, +-2 ulp neighbours,
// each bucket's first pattern and the one below it, the fixed values curve_lut_host.cpp probes that lie in the domain, the ends of both
// NaN ranges; and, for every 64th noise mode, a sweep over the whole domain in steps of 4099 patterns. Between two neighbouring critical
// points either function picks one entry and one segment, so the critical points decide; the sweep is there for what the argument forgot.
// Prints one line "ok curves=<n> checks=<n>" and exits 0, or the first mismatches and exits 1.   (tests/test_lut_nonneg_host.py)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "curve_lut.h"

using namespace musica;

struct F4 { float x, y, z, w; };

static bool same(float a, float b) { return musica_float_bits(a) == musica_float_bits(b); }
static bool in_domain(uint32_t u) { return (u >> 31) == 0u || (u & 0x7FFFFFFFu) > 0x7F800000u; }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s low [low ...]\n", argv[0]); return 2; }
    std::vector<F4> bucket(kLutCap);
    F4 seg[kLutPoints + 1];
    std::vector<uint32_t> pts;
    unsigned long long checks = 0, curves = 0, bad = 0;
    for (int a = 1; a < argc; a++) {
        const float low = strtof(argv[a], nullptr);
        for (uint32_t maxBin = 1; maxBin <= 2048; maxBin++) {
            float x[kLutPoints], y[kLutPoints];
            for (int i = 0; i < kLutPoints; i++) musica_contrast_point(maxBin, low, i, x[i], y[i]);
            const int base = musica_lut_base(x);
            const int n = musica_lut_entries(base);
            if (n <= 0 || base < 0) { if (bad++ < 10) printf("low %g maxBin %u: no table (base %d)\n", low, maxBin, base); continue; }
            int slot[kLutPoints + 3];
            for (int i = 0; i < kLutPoints + 3; i++) slot[i] = i < kLutPoints ? musica_lut_slot(x[i], base) : kLutSlotSentinel;
            for (int k = 0; k < n; k++) musica_lut_entry(x, slot, kLutPoints, k, bucket[k]);
            for (int j = 0; j <= kLutPoints; j++) musica_lut_segment(x, y, kLutPoints, j, seg[j]);
            curves++;
            pts.clear();
            for (int i = 0; i < kLutPoints; i++)
                for (int d = -2; d <= 2; d++) pts.push_back((uint32_t)(musica_float_bits(x[i]) + d));
            for (int key = base - 1; key <= kLutKeyTop + 1; key++) {
                pts.push_back((uint32_t)key << kLutShift);
                pts.push_back(((uint32_t)key << kLutShift) - 1u);
            }
            const uint32_t fixed[] = {0x00000000u, 0x00000001u, 0x00800000u, 0x007FFFFFu, 0x3F800000u, 0x3F7FFFFFu, 0x3F800001u, 0x3FFFFFFFu, 0x40000000u,
                                      0x40000001u, 0x7F7FFFFFu, 0x7F800000u, 0x7F800001u, 0x7FBFFFFFu, 0x7FC00000u, 0x7FFFFFFFu, 0xFF800001u, 0xFFBFFFFFu,
                                      0xFFC00000u, 0xFFFFFFFFu};
            for (uint32_t u : fixed) pts.push_back(u);
            if (maxBin % 64u == 1u) {
                for (uint32_t u = 0u; u < 0x80000000u; u += 4099u) pts.push_back(u);
                for (uint32_t u = 0xFF800001u; u >= 0xFF800001u; u += 4099u) pts.push_back(u);   // ends when u wraps
            }
            for (uint32_t u : pts) {
                if (!in_domain(u)) continue;
                const float s = musica_bits_float((int32_t)u);
                const float got = musica_lut_eval_nonneg(bucket.data(), seg, base, s), want = musica_lut_eval(bucket.data(), seg, base, s);
                checks++;
                if (!same(got, want) && bad++ < 10)
                    printf("low %g maxBin %u s = %a (0x%08x): nonneg %a, general %a\n", low, maxBin, s, (unsigned)u, got, want);
            }
        }
    }
    if (bad) { printf("FAILED: %llu mismatches\n", bad); return 1; }
    printf("ok curves=%llu checks=%llu\n", curves, checks);
    return 0;
}
