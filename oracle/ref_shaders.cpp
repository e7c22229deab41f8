/*
 * ref_shaders.cpp — the reference's on-path compute shaders, compiled for the host.
 * TEST INFRASTRUCTURE ONLY. Built by `make ref` into oracle/_ref/libref_shaders.so (git-ignored).
 *
 * Nothing of the reference is in this file. `make ref` prepares each shaders/X.comp of the reference
 * tree into oracle/_ref/gen/X.inc (prepare_shader.py says exactly what that changes) and this file
 * includes the prepared text, one namespace per shader, behind glsl_host.h. Each extern "C" entry
 * binds the caller's arrays to the shader's images and interface blocks and runs main() once per
 * invocation over groups x local_size, the invocations past the image's edge included.
 *
 * The shaders keep their state in namespace-scope variables (images, blocks, `pointsIndex`), so the
 * entries run one at a time under a lock and reset that state per dispatch.
 * A shader's global with an initialiser (`uint border = 100;`, `vec4 truePixel = ...`, img_relevant.comp:18-26) is
 * initialised per invocation in GLSL and once per process here. That is the same as long as no shader writes such a
 * global. Today exactly one does, `pointsIndex` of gradation_curve_generate.comp:23, and its entry sets it back to the
 * initialiser before each dispatch; a newly hosted shader that writes a global needs the same line in its entry.
 */
#include "glsl_host.h"
#include "../include/musica.h"

#include <cstring>
#include <mutex>

using namespace glsl;

/* The three keyword macros are live only around the prepared shader texts. Every #include of a header, ours or the system's,
 * stays ABOVE this line: none may appear between these #defines and the #undefs below. */
#define float glsl::Float
#define int glsl::I32
#define uint glsl::U32
namespace sh_img_sqrt {
#include "_ref/gen/img_sqrt.inc"
}
namespace sh_img_max_reduce {
#include "_ref/gen/img_max_reduce.inc"
}
namespace sh_min_reduce {
#include "_ref/gen/min_reduce.inc"
}
namespace sh_img_normalize {
#include "_ref/gen/img_normalize.inc"
}
namespace sh_img_smooth {
#include "_ref/gen/img_smooth.inc"
}
namespace sh_img_downsample {
#include "_ref/gen/img_downsample.inc"
}
namespace sh_img_upsample {
#include "_ref/gen/img_upsample.inc"
}
namespace sh_img_smooth_upsampled {
#include "_ref/gen/img_smooth_upsampled.inc"
}
namespace sh_img_difference {
#include "_ref/gen/img_difference.inc"
}
namespace sh_img_sdev {
#include "_ref/gen/img_sdev.inc"
}
namespace sh_noise_hist {
#include "_ref/gen/noise_hist.inc"
}
namespace sh_img_histogram_max {
#include "_ref/gen/img_histogram_max.inc"
}
namespace sh_contrast_curve_generate {
#include "_ref/gen/contrast_curve_generate.inc"
}
namespace sh_contrast_curve_apply {
#include "_ref/gen/contrast_curve_apply.inc"
}
namespace sh_img_cnr {
#include "_ref/gen/img_cnr.inc"
}
namespace sh_noise_reduction {
#include "_ref/gen/noise_reduction.inc"
}
namespace sh_img_addition {
#include "_ref/gen/img_addition.inc"
}
namespace sh_img_relevant {
#include "_ref/gen/img_relevant.inc"
}
namespace sh_gradation_histogram {
#include "_ref/gen/gradation_histogram.inc"
}
namespace sh_gradation_curve_generate {
#include "_ref/gen/gradation_curve_generate.inc"
}
namespace sh_img_apply_gradation_curve {
#include "_ref/gen/img_apply_gradation_curve.inc"
}
namespace sh_noise_hist_render {
#include "_ref/gen/noise_hist_render.inc"
}
namespace sh_gradation_curve_debug_render {
#include "_ref/gen/gradation_curve_debug_render.inc"
}
#undef float
#undef int
#undef uint

namespace {

std::mutex g_lock;

/* groups_x x groups_y workgroups of local_x x local_y invocations, one invocation at a time. */
template <class Main>
void dispatch(uint32_t groups_x, uint32_t groups_y, uint32_t local_x, uint32_t local_y, Main shader_main) {
    gl_NumWorkGroups = uvec3(groups_x, groups_y, 1);
    for (uint32_t wy = 0; wy < groups_y; wy++)
        for (uint32_t wx = 0; wx < groups_x; wx++) {
            gl_WorkGroupID = uvec3(wx, wy, 0);
            for (uint32_t ly = 0; ly < local_y; ly++)
                for (uint32_t lx = 0; lx < local_x; lx++) {
                    gl_LocalInvocationID = uvec3(lx, ly, 0);
                    gl_GlobalInvocationID = uvec3(wx * local_x + lx, wy * local_y + ly, 0);
                    shader_main();
                }
        }
}

/* ceil(side / local size): what covers an image of that side, edge workgroups included. */
uint32_t cover(uint32_t side, uint32_t local) { return (side + local - 1) / local; }

image2D r32f(const float* p, uint32_t side) {
    image2D im;
    im.f32 = const_cast<float*>(p);
    im.w = im.h = (int32_t)side;
    return im;
}
image2D rgba8(uint8_t* p, uint32_t w, uint32_t h) {
    image2D im;
    im.rgba8 = p;
    im.w = (int32_t)w;
    im.h = (int32_t)h;
    return im;
}
uimage1D r32ui(const uint32_t* p, uint32_t n) {
    uimage1D im;
    im.u32 = const_cast<uint32_t*>(p);
    im.n = (int32_t)n;
    return im;
}

/* A curve block of the shaders and the ABI's struct hold the same two floats per point. */
template <class ShaderPoint> void points_in(ShaderPoint* dst, const musica_point* src) {
    static_assert(sizeof(ShaderPoint) == sizeof(musica_point), "Point layout");
    std::memcpy((void*)dst, src, sizeof(musica_point) * MUSICA_MAX_POINTS);
}
template <class ShaderPoint> void points_out(musica_point* dst, const ShaderPoint* src) {
    std::memcpy(dst, (const void*)src, sizeof(musica_point) * MUSICA_MAX_POINTS);
}

#define RUN(ns, gx, gy) dispatch((gx), (gy), ns::local_size_x, ns::local_size_y, ns::main)

}  // namespace

extern "C" {

void ref_img_sqrt(const uint16_t* in, uint32_t side, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_sqrt;
    s::inputImage.u16 = in;
    s::inputImage.w = s::inputImage.h = (int32_t)side;
    s::outputImage = r32f(out, side);
    RUN(s, cover(side, s::local_size_x), cover(side, s::local_size_y));
}

/* One link of a chain: out side = ceil(side / 8). */
void ref_img_max_reduce(const float* in, uint32_t side, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_max_reduce;
    uint32_t os = (side + 7) / 8;
    s::inputImage = r32f(in, side);
    s::outputImage = r32f(out, os);
    RUN(s, cover(os, s::local_size_x), cover(os, s::local_size_y));
}

void ref_min_reduce(const float* in, uint32_t side, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_min_reduce;
    uint32_t os = (side + 7) / 8;
    s::inputImage = r32f(in, side);
    s::outputImage = r32f(out, os);
    RUN(s, cover(os, s::local_size_x), cover(os, s::local_size_y));
}

/* max_image / min_image: the 1 x 1 ends of the two chains. */
void ref_img_normalize(const float* in, uint32_t side, const float* max_image, const float* min_image, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_normalize;
    s::inImage = r32f(in, side);
    s::maxImage = r32f(max_image, 1);
    s::minImage = r32f(min_image, 1);
    s::outImage = r32f(out, side);
    RUN(s, cover(side, s::local_size_x), cover(side, s::local_size_y));
}

void ref_img_smooth(const float* in, uint32_t side, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_smooth;
    s::inputImage = r32f(in, side);
    s::outputImage = r32f(out, side);
    RUN(s, cover(side, s::local_size_x), cover(side, s::local_size_y));
}

void ref_img_smooth_upsampled(const float* in, uint32_t side, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_smooth_upsampled;
    s::inputImage = r32f(in, side);
    s::outputImage = r32f(out, side);
    RUN(s, cover(side, s::local_size_x), cover(side, s::local_size_y));
}

/* out side = ceil(side / 2); dispatched over the output. */
void ref_img_downsample(const float* in, uint32_t side, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_downsample;
    uint32_t os = (side + 1) / 2;
    s::inImage = r32f(in, side);
    s::outImage = r32f(out, os);
    RUN(s, cover(os, s::local_size_x), cover(os, s::local_size_y));
}

/* `out` keeps every texel the shader does not write; dispatched over `dispatch_side` (the reference uses the input's side
 * in the reduce loop and the output's in the expand loop). */
void ref_img_upsample(const float* in, uint32_t in_side, float* out, uint32_t out_side, uint32_t dispatch_side) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_upsample;
    s::inImage = r32f(in, in_side);
    s::outImage = r32f(out, out_side);
    RUN(s, cover(dispatch_side, s::local_size_x), cover(dispatch_side, s::local_size_y));
}

void ref_img_difference(const float* a, const float* b, uint32_t side, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_difference;
    s::inputImageA = r32f(a, side);
    s::inputImageB = r32f(b, side);
    s::outputImage = r32f(out, side);
    RUN(s, cover(side, s::local_size_x), cover(side, s::local_size_y));
}

void ref_img_addition(const float* a, const float* b, uint32_t side, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_addition;
    s::inputImageA = r32f(a, side);
    s::inputImageB = r32f(b, side);
    s::outputImage = r32f(out, side);
    RUN(s, cover(side, s::local_size_x), cover(side, s::local_size_y));
}

void ref_img_sdev(const float* in, uint32_t side, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_sdev;
    s::inputImage = r32f(in, side);
    s::outputImage = r32f(out, side);
    RUN(s, cover(side, s::local_size_x), cover(side, s::local_size_y));
}

/* `groups` workgroups per axis; hist (2048) is accumulated into. */
void ref_noise_hist(const float* sdev, uint32_t side, uint32_t groups, uint32_t* hist) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_noise_hist;
    s::sdevImage = r32f(sdev, side);
    s::histogram = r32ui(hist, MUSICA_NOISE_BINS);
    RUN(s, groups, groups);
}

void ref_img_histogram_max(const uint32_t* hist, uint32_t bins, musica_hist_max_point* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_histogram_max;
    s::histogram = r32ui(hist, bins);
    s::maxValue = out->maxValue;
    s::maxBin = out->maxBin;
    RUN(s, 1, 1);
    out->maxValue = s::maxValue;
    out->maxBin = s::maxBin;
}

/* `curve` goes in as the buffer holds it (stale points stay) and comes out as the shader leaves it. */
void ref_contrast_curve_generate(musica_hist_max_point mp, musica_contrast_params cp, musica_contrast_curve* curve) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_contrast_curve_generate;
    points_in(s::points, curve->points);
    s::pointsCount = curve->pointsCount;
    s::maxValue = mp.maxValue;
    s::maxBin = mp.maxBin;
    s::lowContrastFactor = cp.lowContrastFactor;
    s::highContrastFactor = cp.highContrastFactor;
    RUN(s, 1, 1);
    points_out(curve->points, s::points);
    curve->pointsCount = s::pointsCount;
}

void ref_contrast_curve_apply(const float* band, const float* sdev, uint32_t side, const musica_contrast_curve* curve, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_contrast_curve_apply;
    s::inputImage = r32f(band, side);
    s::sdevImage = r32f(sdev, side);
    s::outputImage = r32f(out, side);
    points_in(s::points, curve->points);
    s::pointsCount = curve->pointsCount;
    RUN(s, cover(side, s::local_size_x), cover(side, s::local_size_y));
}

void ref_img_cnr(const float* sdev, uint32_t side, musica_hist_max_point mp, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_cnr;
    s::sdevImage = r32f(sdev, side);
    s::outputImage = r32f(out, side);
    s::maxValue = mp.maxValue;
    s::maxBin = mp.maxBin;
    RUN(s, cover(side, s::local_size_x), cover(side, s::local_size_y));
}

void ref_noise_reduction(const float* band, uint32_t side, const float* cnr, uint32_t cnr_side, musica_nr_params p, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_noise_reduction;
    s::bandpassImage = r32f(band, side);
    s::cnrImage = r32f(cnr, cnr_side);
    s::outputImage = r32f(out, side);
    s::lowCnr = p.lowCnr;
    s::lowFactor = p.lowFactor;
    s::highCnr = p.highCnr;
    s::highFactor = p.highFactor;
    RUN(s, cover(side, s::local_size_x), cover(side, s::local_size_y));
}

void ref_img_relevant(const float* normalized, uint32_t side, const float* cnr, uint32_t cnr_side, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_relevant;
    s::normalizedImage = r32f(normalized, side);
    s::cnrImage = r32f(cnr, cnr_side);
    s::outputImage = r32f(out, side);
    RUN(s, cover(side, s::local_size_x), cover(side, s::local_size_y));
}

/* `groups` workgroups per axis; hist (1024) is accumulated into. */
void ref_gradation_histogram(const float* img, const float* relevant, uint32_t side, uint32_t groups, uint32_t* hist) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_gradation_histogram;
    s::inputImage = r32f(img, side);
    s::relevantImage = r32f(relevant, side);
    s::histogram = r32ui(hist, MUSICA_GRAD_BINS);
    RUN(s, groups, groups);
}

void ref_gradation_curve_generate(const uint32_t* hist, musica_grad_curve* curve) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_gradation_curve_generate;
    s::histogram = r32ui(hist, MUSICA_GRAD_BINS);
    points_in(s::points, curve->points);
    s::pointsCount = curve->pointsCount;
    s::t0 = curve->t0;
    s::ta = curve->ta;
    s::t1 = curve->t1;
    s::pointsIndex = 0;                                    /* the shader's mutable global: its initialiser, per dispatch */
    RUN(s, 1, 1);
    points_out(curve->points, s::points);
    curve->pointsCount = s::pointsCount;
    curve->t0 = s::t0.v;
    curve->ta = s::ta.v;
    curve->t1 = s::t1.v;
}

void ref_img_apply_gradation_curve(const float* in, uint32_t side, const musica_grad_curve* curve, float* out) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_img_apply_gradation_curve;
    s::inputImage = r32f(in, side);
    s::outputImage = r32f(out, side);
    points_in(s::points, curve->points);
    s::pointsCount = curve->pointsCount;
    RUN(s, cover(side, s::local_size_x), cover(side, s::local_size_y));
}

/* The two plots: one workgroup, a w x h rgba8 image (the caller clears it, as a fresh image is). */
void ref_noise_hist_render(const uint32_t* hist, musica_hist_max_point mp, uint8_t* rgba, uint32_t w, uint32_t h) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_noise_hist_render;
    s::histImage = r32ui(hist, MUSICA_NOISE_BINS);
    s::outputImage = rgba8(rgba, w, h);
    s::maxValue = mp.maxValue;
    s::maxBin = mp.maxBin;
    RUN(s, 1, 1);
}

void ref_gradation_curve_debug_render(const uint32_t* hist, musica_hist_max_point mp, const musica_grad_curve* curve, uint8_t* rgba, uint32_t w, uint32_t h) {
    std::lock_guard<std::mutex> hold(g_lock);
    namespace s = sh_gradation_curve_debug_render;
    s::histImage = r32ui(hist, MUSICA_GRAD_BINS);
    s::outputImage = rgba8(rgba, w, h);
    s::maxValue = mp.maxValue;
    s::maxBin = mp.maxBin;
    points_in(s::points, curve->points);
    s::pointsCount = curve->pointsCount;
    s::t0 = curve->t0;
    s::ta = curve->ta;
    s::t1 = curve->t1;
    RUN(s, 1, 1);
}

}  // extern "C"
