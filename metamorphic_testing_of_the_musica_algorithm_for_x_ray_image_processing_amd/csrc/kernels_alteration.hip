// kernels_alteration.hip — the metamorphic study's alteration generators (harness.py: clamp_translation, clamp_rotate, apply_collimator,
// add_gaussian_noise, apply_quantum_noise; the reference's test/metamorphic_test/script.py:49-141) on the device (musica_alter,
// include/musica.h), and the nearest-neighbour rotation of a reference slot (musica_sim_rotate_reference).
//
// k_alter is one streaming pass: every thread owns kVecBytes / sizeof(T) consecutive pixels of the (dense, row-major) output plane and
// stores them with one 16-byte store (scalar stores when the plane is not a multiple of 16 bytes or not 16-byte aligned). The source is
// read at the same index (copy, noise kinds) or where the geometry maps the pixel (translation, rotation: a gather).
//
// The percentile fills are exact order statistics of a source region, found by a two-pass radix select with no host round trip:
// k_pct_hi counts the high bytes of the region (256 LDS bins per workgroup, added to the global counts), k_pct_lo counts the low
// bytes of the pixels whose high byte is that of the two ranks numpy's 'linear' method interpolates between, and k_pct_finish restates
// numpy 2.2's lerp on the two values in f64. The result stays on the device, where k_alter reads it.
//
// The noise draws come from Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011), keyed by the seed and
// counting (pixel, draw block, stream, 0): a pixel's draws depend on the spec and its index only, never on the launch geometry. Uniform
// doubles are built like numpy's next_double (53 bits from two words); Poisson variates use inversion below lambda = 10 and Hormann's PTRS
// above (W. Hormann, "The transformed rejection method for generating Poisson random variables", 1993), numpy's split; normal variates
// use Box-Muller in f64.
#include <math.h>

#include <algorithm>

#include "kernels_common.h"
#include "launchers.h"

namespace musica {

constexpr int kAlterThreads = 256;
constexpr int kVecBytes = 16;
constexpr int kPctThreads = 256;
constexpr int kPctMaxBlocks = 1024;

// ---- counter-based generator -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t lo0 = 0xD2511F53u * ctr.x, hi0 = __umulhi(0xD2511F53u, ctr.x);
        const uint32_t lo1 = 0xCD9E8D57u * ctr.z, hi1 = __umulhi(0xCD9E8D57u, ctr.z);
        ctr = make_uint4(hi1 ^ ctr.y ^ k0, lo1, hi0 ^ ctr.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return ctr;
}

__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {   // numpy's next_double: [0, 1)
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// The uniform stream of one pixel: block j of its counter gives two doubles.
struct PixelStream {
    uint32_t pixel, stream, k0, k1, j;
    double spare;
    bool have;
    __device__ PixelStream(const AlterDev& a, uint32_t p) : pixel(p), stream(a.stream), k0(a.key0), k1(a.key1), j(0), spare(0.0), have(false) {}
    __device__ double next() {
        if (have) { have = false; return spare; }
        const uint4 r = philox4x32_10(make_uint4(pixel, j++, stream, 0u), k0, k1);
        spare = u53(r.z, r.w);
        have = true;
        return u53(r.x, r.y);
    }
};

// numpy's random_poisson: 0 for lam == 0, inversion (random_poisson_mult) below 10, PTRS (random_poisson_ptrs) from 10 on.
__device__ int poisson_draw(PixelStream& g, double lam) {
    if (!(lam > 0.0)) return 0;
    if (lam < 10.0) {
        const double enlam = exp(-lam);
        double prod = 1.0;
        for (int x = 0; x < 4096; x++) {   // P(k > 4096 | lam < 10) is far below 2^-1000: the bound only keeps the loop finite
            prod *= g.next();
            if (!(prod > enlam)) return x;
        }
        return 4096;
    }
    const double slam = sqrt(lam), loglam = log(lam);
    const double b = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    for (int it = 0; it < 1 << 16; it++) {   // acceptance is above 0.9 per round: the bound only keeps the loop finite
        const double U = g.next() - 0.5;
        const double V = g.next();
        const double us = 0.5 - fabs(U);
        const double kf = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return (int)kf;
        if (kf < 0.0 || (us < 0.013 && V > us)) continue;
        if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -lam + kf * loglam - lgamma(kf + 1.0)) return (int)kf;
    }
    return (int)floor(lam);
}

// mean + sigma * N(0, 1), truncated toward zero like astype(int32) (saturated at the int32 range)
__device__ int gauss_draw(PixelStream& g, double mean, double sigma) {
    const double u1 = 1.0 - g.next();   // (0, 1]
    const double u2 = g.next();
    const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
    const double x = trunc(mean + sigma * z);
    return x >= 2147483647.0 ? 2147483647 : (x <= -2147483648.0 ? (int)-2147483647 - 1 : (int)x);
}

// ---- per-pixel values --------------------------------------------------------------------------------------------------------------
// ndimage.rotate(order=0, mode="constant") of a crop x crop plane (src at the crop's origin, row pitch `pitch`): output pixel (i, j)
// samples input (c0, c1) = (i * m00 + j * m01 + off0, i * m10 + j * m11 + off1), each sum in that order (affine_transform's), is
// `fill` unless 0 <= c <= crop - 1 on both axes, and otherwise the input pixel at floor(c + 0.5).
template <typename T>
__device__ __forceinline__ T rotate_px(const T* __restrict__ src, int pitch, int crop, const AlterDev& a, int i, int j, T fill) {
    const double di = (double)i, dj = (double)j;
    const double c0 = (di * a.m[0] + dj * a.m[1]) + a.off[0];
    const double c1 = (di * a.m[2] + dj * a.m[3]) + a.off[1];
    const double hi = (double)(crop - 1);
    if (!(c0 >= 0.0 && c0 <= hi && c1 >= 0.0 && c1 <= hi)) return fill;
    const int r0 = (int)floor(c0 + 0.5), r1 = (int)floor(c1 + 0.5);
    return src[(size_t)r0 * pitch + r1];
}

template <int KIND, typename T>
__device__ __forceinline__ T alter_px(const T* __restrict__ src, const AlterDev& a, int p, T fill, int32_t* __restrict__ draw) {
    const int n = a.n;
    const int y = p / n, x = p - y * n;
    if (KIND == MUSICA_ALTER_NONE) return src[p];
    if (KIND == MUSICA_ALTER_TRANSLATE) {
        const int oy = y - a.ys, ox = x - a.xs;
        if (oy < 0 || oy >= a.hh || ox < 0 || ox >= a.ww) return fill;
        return src[(size_t)(a.top + oy) * n + a.left + ox];
    }
    if (KIND == MUSICA_ALTER_ROTATE) {
        const int i = y - a.margin, j = x - a.margin;
        if (i < 0 || i >= a.crop || j < 0 || j >= a.crop) return fill;
        return rotate_px<T>(src + (size_t)a.margin * n + a.margin, n, a.crop, a, i, j, fill);
    }
    const uint32_t v = src[p];
    PixelStream g(a, (uint32_t)p);
    if (KIND == MUSICA_ALTER_COLLIMATOR) {
        const bool inside = y >= a.sv && y <= n - a.sv && x >= a.sh && x <= n - a.sh;
        if (inside && !draw) return (T)v;
        const int k = poisson_draw(g, (double)v / 100.0);   // (image / 100).astype(float64) * 1
        if (draw) *draw = k;
        return inside ? (T)v : (T)min(k, 65535);              // float32(k) / float32(1) is exact: k is far below 2^24
    }
    if (KIND == MUSICA_ALTER_GAUSSIAN) {
        const int e = gauss_draw(g, a.mean, a.sigma);
        if (draw) *draw = e;
        const long long s = (long long)v + e;
        return (T)(s < 0 ? 0 : (s > 65535 ? 65535 : s));
    }
    // POISSON: rng.poisson(image.astype(float64) * f).astype(float32) / f — numpy 2 (NEP 50) divides in f32 — clipped, truncated
    const int k = poisson_draw(g, (double)v * a.factor);
    if (draw) *draw = k;
    const float q = (float)k / (float)a.factor;
    return (T)fminf(fmaxf(q, 0.0f), 65535.0f);
}

template <int KIND, typename T>
__global__ __launch_bounds__(kAlterThreads) void k_alter(const T* __restrict__ src, T* __restrict__ out, int32_t* __restrict__ draws, AlterDev a,
                                                        const double* __restrict__ fill_d, int vec) {
    constexpr int V = kVecBytes / sizeof(T);
    const long long total = (long long)a.n * a.n;
    const long long p0 = ((long long)blockIdx.x * kAlterThreads + threadIdx.x) * V;
    if (p0 >= total) return;
    const T fill = fill_d ? (T)(int)*fill_d : (T)0;   // int(np.percentile(...)): a value in [0, 65535], truncated
    union {
        T px[V];
        uint4 v;
    } u;
#pragma unroll
    for (int e = 0; e < V; e++) {
        const long long p = p0 + e;
        if (p < total) u.px[e] = alter_px<KIND, T>(src, a, (int)p, fill, draws ? draws + p : nullptr);
    }
    if (!out) return;
    if (vec) {
        *reinterpret_cast<uint4*>(out + p0) = u.v;
    } else {
        for (int e = 0; e < V && p0 + e < total; e++) out[p0 + e] = u.px[e];
    }
}

template <int KIND, typename T>
static void launch_kind(hipStream_t st, const T* src, T* out, int32_t* draws, const AlterDev& a, const double* fill) {
    constexpr int V = kVecBytes / sizeof(T);
    const long long total = (long long)a.n * a.n;
    const int vec = out && (reinterpret_cast<uintptr_t>(out) % kVecBytes) == 0 && (total % V) == 0;
    const long long threads = (total + V - 1) / V;
    const unsigned blocks = (unsigned)((threads + kAlterThreads - 1) / kAlterThreads);
    hipLaunchKernelGGL((k_alter<KIND, T>), dim3(blocks), dim3(kAlterThreads), 0, st, src, out, draws, a, fill, vec);
}

void launch_alter(hipStream_t st, const uint16_t* src, uint16_t* out, int32_t* draws, const AlterDev& a, const double* fill) {
    switch (a.kind) {
        case MUSICA_ALTER_NONE: launch_kind<MUSICA_ALTER_NONE>(st, src, out, draws, a, fill); break;
        case MUSICA_ALTER_TRANSLATE: launch_kind<MUSICA_ALTER_TRANSLATE>(st, src, out, draws, a, fill); break;
        case MUSICA_ALTER_ROTATE: launch_kind<MUSICA_ALTER_ROTATE>(st, src, out, draws, a, fill); break;
        case MUSICA_ALTER_COLLIMATOR: launch_kind<MUSICA_ALTER_COLLIMATOR>(st, src, out, draws, a, fill); break;
        case MUSICA_ALTER_GAUSSIAN: launch_kind<MUSICA_ALTER_GAUSSIAN>(st, src, out, draws, a, fill); break;
        case MUSICA_ALTER_POISSON: launch_kind<MUSICA_ALTER_POISSON>(st, src, out, draws, a, fill); break;
        default: break;
    }
}

void launch_rotate_u8(hipStream_t st, const uint8_t* src, uint8_t* out, const AlterDev& a) {
    AlterDev r = a;
    r.kind = MUSICA_ALTER_ROTATE;
    r.margin = 0;
    r.crop = a.n;
    launch_kind<MUSICA_ALTER_ROTATE, uint8_t>(st, src, out, nullptr, r, nullptr);
}

// ---- percentile of a region (radix select) -----------------------------------------------------------------------------------------
// hist: [0, 256) high-byte counts, [256, 512) low-byte counts under the lower rank's high byte, [512, 768) under the upper rank's.

struct PctRanks {
    long long r0, r1;   // the ranks numpy interpolates between (equal when the virtual index is at or beyond the last)
    double t;           // gamma
};

// numpy 2.2 _quantile, method 'linear': virtual index (n - 1) * (q / 100); _get_indexes: floor and floor + 1, both the last index when
// the virtual index is >= n - 1 (then the lerp returns that value whatever gamma is).
__device__ __forceinline__ PctRanks pct_ranks(long long n, double q) {
    const double vi = (double)(n - 1) * (q / 100.0);
    PctRanks r;
    if (vi >= (double)(n - 1)) {
        r.r0 = r.r1 = n - 1;
        r.t = 0.0;
    } else {
        const double pf = floor(vi);
        r.r0 = (long long)pf;
        r.r1 = r.r0 + 1;
        r.t = vi - pf;
    }
    return r;
}

// the bin holding rank r of `bins` (256 counts) and the rank inside it
__device__ __forceinline__ int select_bin(const uint32_t* bins, long long r, long long& rest) {
    long long cum = 0;
    for (int b = 0; b < 256; b++) {
        if (cum + bins[b] > r) { rest = r - cum; return b; }
        cum += bins[b];
    }
    rest = 0;
    return 255;
}

__global__ __launch_bounds__(kPctThreads) void k_pct_hi(PctRegion g, uint32_t* __restrict__ hist) {
    __shared__ uint32_t bins[256];
    bins[threadIdx.x] = 0u;
    __syncthreads();
    const long long total = (long long)g.w * g.h;
    for (long long i = (long long)blockIdx.x * kPctThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kPctThreads) {
        const int r = (int)(i / g.w), c = (int)(i - (long long)r * g.w);
        atomicAdd(&bins[g.src[(size_t)(g.y + r) * g.pitch + g.x + c] >> 8], 1u);
    }
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(&hist[threadIdx.x], bins[threadIdx.x]);
}

__global__ __launch_bounds__(kPctThreads) void k_pct_lo(PctRegion g, uint32_t* __restrict__ hist) {
    __shared__ uint32_t bins[2][256];
    __shared__ uint32_t hi[256];
    __shared__ int hb[2];
    bins[0][threadIdx.x] = 0u;
    bins[1][threadIdx.x] = 0u;
    hi[threadIdx.x] = hist[threadIdx.x];   // the scan below reads LDS, not 256 dependent global loads
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long total = (long long)g.w * g.h;
        const PctRanks k = pct_ranks(total, g.q);
        long long rest;
        hb[0] = select_bin(hi, k.r0, rest);
        hb[1] = select_bin(hi, k.r1, rest);
    }
    __syncthreads();
    const int h0 = hb[0], h1 = hb[1];
    const long long total = (long long)g.w * g.h;
    for (long long i = (long long)blockIdx.x * kPctThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kPctThreads) {
        const int r = (int)(i / g.w), c = (int)(i - (long long)r * g.w);
        const uint32_t v = g.src[(size_t)(g.y + r) * g.pitch + g.x + c];
        if ((int)(v >> 8) == h0) atomicAdd(&bins[0][v & 255u], 1u);
        else if ((int)(v >> 8) == h1) atomicAdd(&bins[1][v & 255u], 1u);
    }
    __syncthreads();
    if (bins[0][threadIdx.x]) atomicAdd(&hist[256 + threadIdx.x], bins[0][threadIdx.x]);
    if (bins[1][threadIdx.x]) atomicAdd(&hist[512 + threadIdx.x], bins[1][threadIdx.x]);
}

__global__ __launch_bounds__(kPctThreads) void k_pct_finish(PctRegion g, const uint32_t* __restrict__ gh, double* __restrict__ out) {
    __shared__ uint32_t hist[768];
    for (int i = threadIdx.x; i < 768; i += kPctThreads) hist[i] = gh[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const long long total = (long long)g.w * g.h;
    const PctRanks k = pct_ranks(total, g.q);
    long long rest0, rest1;
    const int h0 = select_bin(hist, k.r0, rest0), h1 = select_bin(hist, k.r1, rest1);
    long long unused;
    const int l0 = select_bin(hist + 256, rest0, unused);
    const int l1 = select_bin(hist + (h1 == h0 ? 256 : 512), rest1, unused);
    const uint32_t a = ((uint32_t)h0 << 8) | (uint32_t)l0, b = ((uint32_t)h1 << 8) | (uint32_t)l1;
    // _lerp: diff = b - a (u16, b >= a); a + diff * t, or b - diff * (1 - t) where t >= 0.5
    const double diff = (double)(uint16_t)(b - a);
    *out = k.t >= 0.5 ? (double)b - diff * (1.0 - k.t) : (double)a + diff * k.t;
}

void launch_percentile(hipStream_t st, const PctRegion& g, uint32_t* hist, double* out) {
    const long long total = (long long)g.w * g.h;
    const unsigned blocks = (unsigned)std::min<long long>(kPctMaxBlocks, std::max<long long>(1, (total + kPctThreads * 16 - 1) / (kPctThreads * 16)));
    hipLaunchKernelGGL(k_pct_hi, dim3(blocks), dim3(kPctThreads), 0, st, g, hist);
    hipLaunchKernelGGL(k_pct_lo, dim3(blocks), dim3(kPctThreads), 0, st, g, hist);
    hipLaunchKernelGGL(k_pct_finish, dim3(1), dim3(kPctThreads), 0, st, g, hist, out);
}

}  // namespace musica
