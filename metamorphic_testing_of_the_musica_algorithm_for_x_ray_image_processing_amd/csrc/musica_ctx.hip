// musica_ctx.hip — host side of libmusica_hip.so: the context that replaces class VulkanProcessing
// (include/vk_processing.h:26-356 of the reference): create / destroy, queries, getters, dumps, profiling
// and the bench entry points of include/musica.h (the step itself: musica_step.hip). No CPU fallback
// exists: without a HIP device musica_create fails loudly.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>

#include "musica_ctx.h"

// host-only helpers implemented in musica_io.cpp
extern "C" int musica_write_bmp_gray(const char* path, uint32_t w, uint32_t h, const uint8_t* data);
extern "C" uint32_t musica_bmp24_header(uint32_t w, uint32_t h, uint8_t hdr[54]);
extern "C" int musica_write_file(const char* path, const uint8_t* bytes, size_t count);

// ---- errors ---------------------------------------------------------------------------
static thread_local std::string g_last_error;

int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    fprintf(stderr, "MUSICA ERROR: %s\n", buf);  // cf. "VK STATE ERROR: %s" src/vk_processing.cpp:14-18
    return 0;
}

// MUSICA_TIMING=1: where the host-side time of create / save goes, one line per phase on stderr (the drop-in CLI is one process per
// image: its wall time is start-up, allocation and file I/O, not the pipeline)
struct Tick {
    bool on;
    std::chrono::high_resolution_clock::time_point t;
    const char* what;
    explicit Tick(const char* w) : on(env_int("MUSICA_TIMING", 0) != 0), t(std::chrono::high_resolution_clock::now()), what(w) {}
    void lap(const char* phase) {
        if (!on) return;
        const auto n = std::chrono::high_resolution_clock::now();
        fprintf(stderr, "[musica timing] %s: %s %.2f ms\n", what, phase, std::chrono::duration<float, std::milli>(n - t).count());
        t = n;
    }
};

// highContrastFactor / lowContrastFactor per level: src/vk_processing.cpp:259-293, both forms of each (the reference picks one per
// #define LINEAR_*_CONTRAST_LEVELS_REDUCTION, include/vk_processing.h:16-17; musica_tunables carries the choice).
static musica_contrast_params host_contrast_params(uint32_t i, uint32_t levels, const musica_tunables& t) {
    const uint32_t coarserLevelsStart = MUSICA_COARSER_LEVELS_START;
    const float highContrastMaxReduction = t.high_contrast_max_reduction, lowContrastMaxEnhancment = t.low_contrast_max_enhancement;  // vk_processing.h:48-49
    musica_contrast_params cp;
    const uint32_t coarserLevelsCount = levels - coarserLevelsStart;
    if (i < coarserLevelsStart) cp.highContrastFactor = 1.0f;
    else if (t.linear_high_contrast) {
        // :264-268 — divides by (pyramidLevels - coarserLevelsStart - 1): 0 / 0 at L = 4, taken as "no reduction" like the power form's exponent 0
        cp.highContrastFactor = coarserLevelsCount > 1
            ? 1.0f - (float)(i - coarserLevelsStart) * (1.0f - highContrastMaxReduction) / (float)(levels - coarserLevelsStart - 1) : 1.0f;
    } else {
        // the reference divides by (coarserLevelsCount - 1): 0/0 at L = 4 — taken as exponent 0 there
        const float e = coarserLevelsCount > 1 ? (float)(i - coarserLevelsStart) / (float)(coarserLevelsCount - 1) : 0.0f;
        cp.highContrastFactor = powf(highContrastMaxReduction, e);
    }
    if (i >= coarserLevelsStart) cp.lowContrastFactor = 1.0f;
    else if (t.linear_low_contrast) cp.lowContrastFactor = lowContrastMaxEnhancment - (float)i * ((lowContrastMaxEnhancment - 1.0f) / (float)coarserLevelsStart);   // :284-286
    else cp.lowContrastFactor = powf(lowContrastMaxEnhancment, 1.0f - ((float)i / (float)coarserLevelsStart));   // :289-291
    return cp;
}

// src/vk_processing.cpp:321-325; the buffer bound to band level l is index l (:1518-1520).
static musica_nr_params host_nr_params(uint32_t i, const musica_tunables& t) {
    const float nrHighCnr = t.nr_high_cnr, nrMaxHighFactor = t.nr_max_high_factor, nrLowCnr = t.nr_low_cnr, nrMinLowFactor = t.nr_min_low_factor;  // vk_processing.h:39-42
    musica_nr_params q;
    q.highCnr = nrHighCnr;
    q.highFactor = nrMaxHighFactor - (nrMaxHighFactor - 1.0f) * ((float)i / (float)MUSICA_CNR_LEVEL);
    q.lowCnr = nrLowCnr;
    q.lowFactor = nrMinLowFactor + (1.0f - nrMinLowFactor) * ((float)i / (float)MUSICA_CNR_LEVEL);
    return q;
}

extern "C" {

uint32_t musica_abi_version(void) { return MUSICA_ABI_VERSION; }
const char* musica_last_error(void) { return g_last_error.c_str(); }

int musica_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void musica_destroy(musica_ctx* c) {
    if (!c) return;
    hipSetDevice(c->p.device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (int k = 0; k < kLaneStreams; k++) if (c->lane_stream[k]) hipStreamSynchronize(c->lane_stream[k]);
    for (musica_ctx* v : c->lanes) {
        for (auto& sp : v->spans) { hipEventDestroy(sp.a); hipEventDestroy(sp.b); }
        for (int k = 0; k < kGraphSlots; k++) if (v->graph_exec[k]) hipGraphExecDestroy(v->graph_exec[k]);
        delete v;
    }
    for (int k = 0; k < kLaneStreams; k++) {
        if (c->lane_stream[k]) { hipStreamSynchronize(c->lane_stream[k]); hipStreamDestroy(c->lane_stream[k]); }
        if (c->lane_done[k]) hipEventDestroy(c->lane_done[k]);
    }
    if (c->lane_start) hipEventDestroy(c->lane_start);
    for (int k = 0; k < 2; k++) if (c->lane_copy[k]) { hipStreamSynchronize(c->lane_copy[k]); hipStreamDestroy(c->lane_copy[k]); }
    for (hipEvent_t e : c->img_copied) hipEventDestroy(e);
    if (c->copy_stream) { hipStreamSynchronize(c->copy_stream); hipStreamDestroy(c->copy_stream); }
    for (int k = 0; k < 2; k++) {
        if (c->ev_copied[k]) hipEventDestroy(c->ev_copied[k]);
        if (c->ev_consumed[k]) hipEventDestroy(c->ev_consumed[k]);
    }
    for (auto& s : c->spans) { hipEventDestroy(s.a); hipEventDestroy(s.b); }
    for (void* p : c->allocations) hipFree(p);
    if (c->h_out8) hipHostFree(c->h_out8);
    if (c->h_bmp) hipHostFree(c->h_bmp);
    for (int k = 0; k < kGraphSlots; k++) if (c->graph_exec[k]) hipGraphExecDestroy(c->graph_exec[k]);
    if (c->side) { hipStreamSynchronize(c->side); hipStreamDestroy(c->side); }
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_join) hipEventDestroy(c->ev_join);
    if (c->ev_caller) hipEventDestroy(c->ev_caller);
    if (c->ev_signal) hipEventDestroy(c->ev_signal);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

static musica_ctx* create_impl(const musica_params* params, const musica_tunables* tunables);
void musica_tunables_default(musica_tunables* t) {
    if (!t) return;
    t->nr_high_cnr = 9.0f; t->nr_max_high_factor = 1.2f; t->nr_low_cnr = 3.0f; t->nr_min_low_factor = 0.6f;   // include/vk_processing.h:39-42
    t->high_contrast_max_reduction = 0.2f; t->low_contrast_max_enhancement = 3.0f;                             // :48-49
    t->linear_low_contrast = 0u; t->linear_high_contrast = 0u;                                                 // :16-17 (commented out)
}
int musica_get_tunables(const musica_ctx* c, musica_tunables* out) {
    if (!c || !out) return fail("musica_get_tunables: NULL argument");
    *out = c->tun;
    return 1;
}
musica_ctx* musica_create(const musica_params* params) { return musica_create_ex(params, nullptr); }
musica_ctx* musica_create_ex(const musica_params* params, const musica_tunables* tunables) {
    try {
        return create_impl(params, tunables);
    } catch (const std::exception& e) {
        fail("musica_create: %s", e.what());
    } catch (...) {
        fail("musica_create: unknown C++ exception");
    }
    return nullptr;
}

static musica_ctx* create_impl(const musica_params* params, const musica_tunables* tunables) {
    if (!params) { fail("musica_create: params is NULL"); return nullptr; }
    {   // a per-image buffer the visitor does not name would be neither allocated nor moved to a lane's images
        musica_ctx probe{};
        if (for_each_buffer(probe, probe, [](auto&, size_t) {}) != sizeof(DeviceBuffers) / sizeof(void*)) {
            fail("musica_create: for_each_buffer does not visit every member of DeviceBuffers");
            return nullptr;
        }
    }
    musica_tunables tun;
    musica_tunables_default(&tun);
    if (tunables) {
        tun = *tunables;
        const float v[6] = {tun.nr_high_cnr, tun.nr_max_high_factor, tun.nr_low_cnr, tun.nr_min_low_factor, tun.high_contrast_max_reduction, tun.low_contrast_max_enhancement};
        for (float x : v)
            if (!(x == x) || x > 3.0e38f || x < -3.0e38f) { fail("musica_create_ex: a tunable is not a finite number"); return nullptr; }
        if (tun.nr_high_cnr == tun.nr_low_cnr) { fail("musica_create_ex: nr_high_cnr == nr_low_cnr (the slope of linearFunction, noise_reduction.comp:28, divides by their difference)"); return nullptr; }
    }
    const uint32_t N = params->image_size;
    // 16384: a level-0 f32 plane is then 1 GiB — the kernels address planes through buffer descriptors with 32-bit
    // byte offsets and use bit 31 as the "nothing to load" marker, so a plane must stay below 2 GiB
    if (N < 16 || N > 16384) { fail("musica_create: image_size %u out of range [16, 16384]", N); return nullptr; }
    uint32_t Lref = 0;
    while ((1u << Lref) < N) Lref++;  // pyramidLevels = ceil(log2(imageSize)), src/vk_processing.cpp:1989
    const uint32_t L = params->levels ? params->levels : Lref;
    if (L < MUSICA_MIN_LEVELS || L > Lref || L > MUSICA_MAX_LEVELS) {
        fail("musica_create: levels %u out of range [%d, %u] for image_size %u", L, MUSICA_MIN_LEVELS, Lref, N);
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fail("musica_create: no HIP device available (this library has no CPU path)");
        return nullptr;
    }
    if (params->device < 0 || params->device >= ndev) { fail("musica_create: device %d out of range (%d devices)", params->device, ndev); return nullptr; }
    if (hipSetDevice(params->device) != hipSuccess) { fail("musica_create: hipSetDevice(%d) failed", params->device); return nullptr; }

    musica_ctx* c = new musica_ctx();
    c->p = *params;
    if (c->p.flags & MUSICA_FLAG_ONE_SHOT) c->p.flags |= MUSICA_FLAG_NO_AUTOTUNE | MUSICA_FLAG_NO_GRAPH;
    params = &c->p;
    c->tun = tun;
    c->N = (int)N; c->L = (int)L; c->B = params->batch ? (int)params->batch : 1;
    c->p.levels = L; c->p.batch = (uint32_t)c->B;
    c->ref_order = (params->flags & MUSICA_FLAG_REFERENCE_ORDER) ? 1 : 0;
    c->generic = (params->flags & MUSICA_FLAG_GENERIC_KERNELS) != 0 || c->ref_order;   // the literal order lives in the one-thread-per-texel kernels
    int s = (int)N;
    for (int i = 0; i <= c->L; i++) {
        c->lv[i].S = s;
        c->lv[i].pitch = round_up4(s);
        c->lv[i].plane = (size_t)c->lv[i].pitch * s;
        s = (s + 1) / 2;  // ceil(currentImageSize / 2.0f), src/vk_processing.cpp:116,150
    }
    { uint32_t n = N; while (n % 8 == 0) n /= 8; c->min_chain_exact = (n == 1); }
    c->hist_cov = (int)(N / 512u) * 512;  // imageSize / histWorkgroupCoverage groups, src/vk_processing.cpp:2293-2295
    for (int i = 0; i < c->L; i++) c->h_cparams[i] = host_contrast_params((uint32_t)i, L, c->tun);
    for (int i = 0; i < 3; i++) c->h_nr[i] = host_nr_params((uint32_t)i, c->tun);
    c->expand_rows = env_int("MUSICA_EXPAND_ROWS", 8);
    c->sdev_rows = env_int("MUSICA_SDEV_ROWS", 32) & ~15;
    if (c->sdev_rows < 16) c->sdev_rows = 16;
    c->grad_groups = 1;

    const size_t B = (size_t)c->B;
    // How a step is dispatched (DESIGN.md section 4 has the measurements behind every line; musica_get_dispatch reports the choice):
    //  * MUSICA_FLAG_LINEAR: ONE in-order stream in the reference's order, replayed as a graph — the form for contexts whose steps
    //    run beside other contexts' steps (musica_pipeline_*): such a context creates one stream, so that the runtime's round-robin
    //    puts consecutive contexts on different hardware queues (4 by default) and nothing of a step waits for another queue;
    //  * a context that runs alone with a small step — one image below 2048^2, or a batch of up to 3072^2 texels — is mostly
    //    launches smaller than their fixed cost: eager launches on one stream (a graph node costs more than a kernel launched behind
    //    its predecessor, a cross-stream join more than it hides: 512^2 0.081 ms against 0.116 for three streams + graph, 1024^2
    //    0.100 / 0.131, 8 x 1024^2 0.170 / 0.196, 2 x 2048^2 0.180 / 0.207);
    //  * everything larger: TWO streams (enqueue_two_streams: the analysis launches beside the reduce tail and the constant-gain expand
    //    slots, one fork and one join), replayed as a graph (2048^2 L6 0.138 against 0.142 on one stream, 4096^2 L8 + CLAHE 0.306 /
    //    0.319, 8192^2 L10 0.747 / 0.779, 4 x 2048^2 0.264 / 0.263 (three streams: 0.287), 2 x 4096^2 0.433 / 0.457 (0.451), 8 x 2048^2
    //    0.434 / 0.443 (0.431)); one image with a pyramid of 11 or more levels: eager (3072^2 L12 0.214 against 0.220 as a graph and
    //    0.240 on one stream, 4096^2 L12 0.277 / 0.292 / 0.308);
    //  * one-shot contexts (MUSICA_FLAG_ONE_SHOT: musica-standalone): one stream — creating a second one costs more than one step saves;
    //  (The three-stream script and the image groups of rounds 1 - 3 won nowhere by more than noise at the end of round 3 and left in round 4.)
    const bool lone = !(params->flags & MUSICA_FLAG_LINEAR);
    const bool one_shot = (params->flags & MUSICA_FLAG_ONE_SHOT) != 0;
    const bool small_step = c->B == 1 ? N < 2048 : (size_t)c->B * N * N <= (size_t)3072 * 3072;
    c->dag = !lone ? 0 : (env_int("MUSICA_STREAMS", (small_step || one_shot) ? 1 : 2) >= 2 ? 2 : 0);
    c->use_graph = !(params->flags & MUSICA_FLAG_NO_GRAPH) && env_int("MUSICA_GRAPH", (lone && (small_step || (c->B == 1 && L >= 11))) ? 0 : 1) != 0;
    Tick tick("create");
    bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
    if (c->dag) {
        ok = ok && hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) == hipSuccess;
    }
    c->fuse_u16 = (N % 8) == 0 && !c->generic;
    // fused gradation histogram: streaming level-0 kernels on raw pixels, cnr scale 8 (every N >= 57 with N % 8 == 0), no CLAHE
    // block (it wants the stored relevant image anyway)
    // (a CLAHE context fuses too since its relevant image comes from the raw pixels, k_relevant4<true>; MUSICA_CLAHE_FUSE=0: as before)
    c->clahe_raw = (params->flags & MUSICA_FLAG_CLAHE) && c->fuse_u16 && (N % 4) == 0 && env_int("MUSICA_CLAHE_FUSE", 1) != 0 &&
                   (cnr_scale(c->lv[0].S, c->lv[MUSICA_CNR_LEVEL].S) % 4) == 0;
    c->clahe_in_expand = env_int("MUSICA_CLAHE_IN_EXPAND", 1) != 0;
    c->clahe_one_apply = env_int("MUSICA_CLAHE_ONE_APPLY", 1) != 0;
    c->tiny_tail = env_int("MUSICA_TINY_TAIL", 1) != 0;
    c->grad_one_launch = env_int("MUSICA_GRAD_ONE_LAUNCH", 1) != 0;
    c->xcd_swizzle = env_int("MUSICA_XCD_SWIZZLE", 1) != 0 ? 1 : 0;
    c->xcd_regions = env_int("MUSICA_XCD_REGIONS", 1) != 0 ? 1 : 0;
    {
        // sdev computed inside the expand launches of levels 0 .. 2 (k_expand_fast<.., SD>) instead of stored by the sdev launch and read back:
        // 8 of a step's 48 bytes per input pixel against ~35 % more vector work in those expand launches. It pays where a step is bound by its
        // bytes — steps in flight (the contexts of a pipeline: MUSICA_FLAG_LINEAR) from 2 x 2048^2 texels per step, a lone context from
        // 8 x 2048^2 (same-box A/B, three steps in flight / one context: 8 x 2048^2 -7.8 % / -0.8 %, 8192^2 -12.4 % / -5.7 %, 4 x 2048^2
        // -2.6 %, 3072^2 L12 -5.0 % / +4.1 %, 4096^2 + CLAHE -1.5 % / +2.5 %, one 2048^2 image +2.5 % / +6.6 %). MUSICA_SDEV_IN_EXPAND=0 | 1 overrides.
        const size_t texels = (size_t)c->B * N * N;
        const bool pays = texels >= ((params->flags & MUSICA_FLAG_LINEAR) ? (size_t)2 : (size_t)8) * 2048 * 2048;
        c->sd_fused = env_int("MUSICA_SDEV_IN_EXPAND", pays ? 1 : 0) != 0 && !c->generic;
    }
    // every level's sdev pass in one launch for batches and for the contexts of a pipeline (same-box A/B: a lone 8 x 2048^2 context -3.5 %, 8192^2 -1.1 %;
    // three steps in flight 8 x 2048^2 -1 %, 8192^2 -1.5 %, 3072^2 L12 -3.5 %); a lone context with one image keeps one launch per marching level:
    // beside the reduce tail of its two-stream script the merged launch slows the tail's small launches (3072^2 L12 +4 %, 2048^2 +0.7 %)
    // the pairs of the one-stream script (k_rb_sdev) for the contexts of a pipeline from 2 x 2048^2 texels per step (same-box A/B, three steps in flight:
    // 8 x 2048^2 -3.1 %, 8192^2 -2.0 %, 4096^2 + CLAHE -2.1 %, 3072^2 L12 +0.6 %, one 2048^2 image +2.8 %); a lone one-stream context is slower with them
    // (512^2 +17 %, 1024^2 +3 %, 1536^2 +7 %, 2 / 4 x 1024^2 +5 / +4 %): alone on the chip a pair costs what its two launches cost one after the other
    c->pair_rb_sdev = env_int("MUSICA_PAIR_RB_SDEV", ((params->flags & MUSICA_FLAG_LINEAR) && (size_t)c->B * N * N >= (size_t)2 * 2048 * 2048) ? 1 : 0) != 0;
    c->hist_in_rb = env_int("MUSICA_HIST_IN_RB", -1);
    c->hist_rb_rows = env_int("MUSICA_HIST_RB_ROWS", 0) & ~7;
    c->sdev_one_launch = env_int("MUSICA_SDEV_ONE_LAUNCH", ((params->flags & MUSICA_FLAG_LINEAR) || c->B > 1) ? 1 : 0) != 0;
    c->fuse_gh = env_int("MUSICA_FUSE_GH", 1) != 0 && c->fuse_u16 && (!(params->flags & MUSICA_FLAG_CLAHE) || c->clahe_raw) &&
                 cnr_scale(c->lv[0].S, c->lv[MUSICA_CNR_LEVEL].S) == 8;
    tick.lap("streams + events");
    for_each_buffer(*c, *c, [&](auto& ptr, size_t count) { if (count) ok = ok && dalloc(c, &ptr, B * count); });
    ok = ok && dalloc(c, &c->d_cparams, (size_t)L);
    ok = ok && dalloc(c, &c->d_plot, (size_t)MUSICA_HIST_RENDER_WIDTH * MUSICA_HIST_RENDER_HEIGHT);
    tick.lap("device buffers");
    ok = ok && hipMemcpy(c->d_cparams, c->h_cparams, sizeof(musica_contrast_params) * L, hipMemcpyHostToDevice) == hipSuccess;
    tick.lap("parameter upload");
    if (!ok) {
        fail("musica_create: device allocation failed (%s)", hipGetErrorString(hipGetLastError()));
        musica_destroy(c);
        return nullptr;
    }
    c->cur_input = c->d_input;
    c->cur = c->stream;
    default_rows(c, c->B);
    const bool tune = !(params->flags & MUSICA_FLAG_NO_AUTOTUNE) && env_int("MUSICA_AUTOTUNE", 1) && !c->generic;
    if (tune) autotune(c);
    return c;
}

uint32_t musica_get_image_size(const musica_ctx* c) { return c ? (uint32_t)c->N : 0; }
uint32_t musica_get_levels(const musica_ctx* c) { return c ? (uint32_t)c->L : 0; }
uint32_t musica_get_batch(const musica_ctx* c) { return c ? (uint32_t)c->B : 0; }
int musica_get_dispatch(const musica_ctx* c, int* streams, int* graph) {
    if (!c) return 0;
    if (streams) *streams = c->dag == 0 ? 1 : 2;
    if (graph) *graph = c->use_graph ? 1 : 0;
    return 1;
}
int musica_fuses_gradation_histogram(const musica_ctx* c) { return (c && c->fuse_gh && !c->generic) ? 1 : 0; }
int musica_fuses_reduce_band(const musica_ctx* c) { return (c && rb_level(c, 0)) ? 1 : 0; }
int musica_fuses_sdev(const musica_ctx* c) { return (c && c->sd_fused && rb_level(c, 0)) ? 1 : 0; }
int musica_fuses_noise_hist(const musica_ctx* c) { return (c && step_form(c, STEP_WHOLE).hist_rows > 0) ? 1 : 0; }
int musica_get_paired_levels(const musica_ctx* c) { return c ? step_form(c, STEP_WHOLE).pairs : 0; }
uint32_t musica_get_level_size(const musica_ctx* c, uint32_t level) { return (c && (int)level <= c->L) ? (uint32_t)c->lv[level].S : 0; }

}  // extern "C"

// pitched device plane -> dense host image
static int download_plane(musica_ctx* c, const float* d_plane, const LevelDesc& l, float* dst) {
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy2D(dst, (size_t)l.S * sizeof(float), d_plane, (size_t)l.pitch * sizeof(float), (size_t)l.S * sizeof(float), (size_t)l.S,
                       hipMemcpyDeviceToHost));
    return 1;
}
static int upload_plane(musica_ctx* c, float* d_plane, const LevelDesc& l, const float* src) {
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy2D(d_plane, (size_t)l.pitch * sizeof(float), src, (size_t)l.S * sizeof(float), (size_t)l.S * sizeof(float), (size_t)l.S,
                       hipMemcpyHostToDevice));
    return 1;
}

template <typename T>
static int download_small(musica_ctx* c, const T* d_src, T* dst, size_t count) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(dst, d_src, count * sizeof(T), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail("device read-back failed: %s", hipGetErrorString(e));
    return 1;
}

extern "C" {

const uint16_t* musica_input_device_ptr(musica_ctx* c) { return c ? c->d_input : nullptr; }

void* musica_host_alloc(musica_ctx* c, size_t bytes) {
    if (!c || hipSetDevice(c->p.device) != hipSuccess) return nullptr;
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { fail("musica_host_alloc(%zu) failed", bytes); return nullptr; }
    return p;
}
void musica_host_free(musica_ctx* c, void* p) {
    if (!c || !p) return;
    hipSetDevice(c->p.device);
    hipStreamSynchronize(c->stream);
    if (c->copy_stream) hipStreamSynchronize(c->copy_stream);
    hipHostFree(p);
}

uint32_t musica_image_side(const musica_ctx* c, musica_image_kind kind, uint32_t level) {
    if (!c) return 0;
    switch (kind) {
        case MUSICA_IMG_NORMALIZED: case MUSICA_IMG_GRADED: case MUSICA_IMG_RELEVANT: case MUSICA_IMG_SQRT: case MUSICA_IMG_CLAHE_GRADED:
            return level == 0 ? (uint32_t)c->N : 0;
        case MUSICA_IMG_CNR: return level == MUSICA_CNR_LEVEL ? (uint32_t)c->lv[MUSICA_CNR_LEVEL].S : 0;
        case MUSICA_IMG_DOWNSAMPLED: return (int)level < c->L ? (uint32_t)c->lv[level + 1].S : 0;
        case MUSICA_IMG_BANDPASS: case MUSICA_IMG_SDEV: case MUSICA_IMG_EXPAND: case MUSICA_IMG_LOWPASS: case MUSICA_IMG_EXP_BANDPASS: case MUSICA_IMG_CONTRAST_BAND:
            return (int)level < c->L ? (uint32_t)c->lv[level].S : 0;
        default: return 0;
    }
}

// The plane of image idx that a step stores for (kind, level), and its level; null for the kinds computed on demand and for a buffer
// this context does not have. The caller has checked (kind, level) with musica_image_side.
static float* stored_plane(musica_ctx* c, uint32_t idx, musica_image_kind kind, uint32_t level, const LevelDesc** desc) {
    float* const* buf = nullptr;
    switch (kind) {
        case MUSICA_IMG_NORMALIZED: buf = &c->d_norm; level = 0; break;
        case MUSICA_IMG_GRADED: buf = &c->d_graded; level = 0; break;
        case MUSICA_IMG_CLAHE_GRADED: buf = &c->d_clahe_graded; level = 0; break;
        case MUSICA_IMG_CNR: buf = &c->d_cnr; level = MUSICA_CNR_LEVEL; break;
        case MUSICA_IMG_DOWNSAMPLED: buf = &c->d_down[level]; level++; break;
        case MUSICA_IMG_BANDPASS: buf = &c->d_band[level]; break;
        case MUSICA_IMG_EXPAND: buf = &c->d_recon[level]; break;
        case MUSICA_IMG_SDEV: if (level <= MUSICA_CNR_LEVEL) buf = &c->d_sdev[level]; break;
        default: break;
    }
    *desc = &c->lv[level];
    return buf && *buf ? image_slice(c, *buf, idx) : nullptr;
}

// Resolves (kind, level) to a device plane of image `idx`; on-demand kinds are computed into d_scratch.
static int resolve_image(musica_ctx* c, uint32_t idx, musica_image_kind kind, uint32_t level, const float** plane, const LevelDesc** desc) {
    if (musica_image_side(c, kind, level) == 0) return fail("musica_get_image: no image kind=%d level=%u", (int)kind, level);
    if (kind == MUSICA_IMG_NORMALIZED) ensure_normalized(c);
    if (kind == MUSICA_IMG_SDEV) ensure_sdev(c);
    if ((*plane = stored_plane(c, idx, kind, level, desc))) return 1;
    const LevelDesc& l0 = c->lv[0];
    const LevelDesc& l3 = c->lv[MUSICA_CNR_LEVEL];
    switch (kind) {
        case MUSICA_IMG_CLAHE_GRADED: return fail("musica_get_image: ctx was created without MUSICA_FLAG_CLAHE");
        case MUSICA_IMG_SDEV:
            // levels >= 4: the reference never writes these images (src/vk_processing.cpp:2285) -> zeros (Q2)
            HIP_OK(hipMemsetAsync(c->d_scratch, 0, c->lv[level].plane * sizeof(float), c->stream));
            *plane = c->d_scratch; return 1;
        case MUSICA_IMG_RELEVANT:
            ensure_normalized(c);
            launch_relevant(c->stream, c->d_norm, c->d_cnr, c->d_scratch, l0, l3, (int)cnr_scale(l0.S, l3.S), c->B);
            *plane = c->d_scratch + idx * l0.plane; *desc = &c->lv[0]; return 1;
        case MUSICA_IMG_SQRT:
            launch_sqrt(c->stream, c->cur_input, c->d_scratch, l0, c->B);
            *plane = c->d_scratch + idx * l0.plane; *desc = &c->lv[0]; return 1;
        case MUSICA_IMG_LOWPASS:  // lowpassImageStates[level] = smooth_upsampled(upsample(downsampled[level]))
            launch_lowpass(c->stream, c->d_down[level], c->d_scratch, c->lv[level], c->lv[level + 1], c->B, c->ref_order);
            *plane = c->d_scratch + idx * c->lv[level].plane; *desc = &c->lv[level]; return 1;
        case MUSICA_IMG_EXP_BANDPASS: case MUSICA_IMG_CONTRAST_BAND: {
            ensure_sdev(c);
            const ExpandArgs a = expand_args(c, step_form(c, STEP_STAGE), (int)level, c->d_scratch);
            launch_exp_band(c->stream, a, gain_mode((int)level), kind == MUSICA_IMG_EXP_BANDPASS && uses_nr((int)level), c->B);
            *plane = c->d_scratch + idx * c->lv[level].plane; *desc = &c->lv[level]; return 1;
        }
        default: return fail("musica_get_image: unsupported kind %d", (int)kind);
    }
}

int musica_get_image(musica_ctx* c, uint32_t idx, musica_image_kind kind, uint32_t level, float* dst) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    if (!dst) return fail("musica_get_image: dst is NULL");
    const float* plane = nullptr;
    const LevelDesc* d = nullptr;
    if (!resolve_image(c, idx, kind, level, &plane, &d)) return 0;
    return download_plane(c, plane, *d, dst);
}

int musica_debug_set_image(musica_ctx* c, uint32_t idx, musica_image_kind kind, uint32_t level, const float* src) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    if (!src) return fail("musica_debug_set_image: src is NULL");
    if (musica_image_side(c, kind, level) == 0) return fail("musica_debug_set_image: no image kind=%d level=%u", (int)kind, level);
    if (kind == MUSICA_IMG_NORMALIZED && c->fuse_u16)
        return fail("musica_debug_set_image: the normalized image is not stored on the hot path (level 0 reads the raw pixels)");
    if (kind == MUSICA_IMG_SDEV && level > MUSICA_CNR_LEVEL) return fail("musica_debug_set_image: sdev exists only for levels 0..3");
    const LevelDesc* d = nullptr;
    float* plane = kind == MUSICA_IMG_CLAHE_GRADED ? nullptr : stored_plane(c, idx, kind, level, &d);   // the CLAHE output is never set
    if (!plane) return fail("musica_debug_set_image: kind %d is not stored on the hot path", (int)kind);
    // the stored sdev images first (every level: the step's, computed from the step's band images): a later getter must not overwrite
    // an sdev image the caller sets here, nor rebuild the step's sdev images from a band image the caller sets here
    if (kind == MUSICA_IMG_SDEV || kind == MUSICA_IMG_BANDPASS) ensure_sdev(c);
    return upload_plane(c, plane, *d, src);
}

int musica_get_graded(musica_ctx* c, float* dst) {
    CHECK_CTX(c);
    if (!dst) return fail("musica_get_graded: dst is NULL");
    for (int b = 0; b < c->B; b++)
        if (!download_plane(c, image_slice(c, c->d_graded, b), c->lv[0], dst + (size_t)b * c->N * c->N)) return 0;
    return 1;
}

// saveOutImage: crop margin 10, (uint8_t)(255.0f * (v - 0) / (1 - 0)) (src/vk_processing.cpp:2624-2634) — on the device
// (k_out_pixels), then (N - 20)^2 bytes into pinned host memory: 1 B per output pixel instead of the reference's 4 B per input
// pixel through pageable memory (loadDataFromImage, src/vk_state.cpp:777-803). Returns the pinned buffer (valid until the next call).
static const uint8_t* out_pixels_pinned(musica_ctx* c, uint32_t idx) {
    const uint32_t N = (uint32_t)c->N, margin = MUSICA_OUT_MARGIN;
    if (N <= 2 * margin) { fail("saveOutImage: image too small for the %u-pixel margin", margin); return nullptr; }
    const size_t nw = N - 2 * margin, bytes = nw * nw;
    Tick tick("save");
    if (!c->h_out8) {   // keyed on the LAST resource of the block: a call that failed half-way is retried, never half-initialised
        if (!ensure(c, &c->d_out8, bytes)) { fail("saveOutImage: device allocation failed"); return nullptr; }
        if (hipHostMalloc((void**)&c->h_out8, bytes, hipHostMallocDefault) != hipSuccess) { c->h_out8 = nullptr; fail("saveOutImage: pinned allocation failed"); return nullptr; }
    }
    tick.lap("device + pinned buffers");
    launch_out_pixels(c->stream, image_slice(c, c->d_graded, idx), c->lv[0], (int)margin, c->d_out8);
    hipError_t e = hipMemcpyAsync(c->h_out8, c->d_out8, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { fail("saveOutImage: read-back failed: %s", hipGetErrorString(e)); return nullptr; }
    tick.lap("crop + quantise kernel, read-back");
    return c->h_out8;
}

int musica_get_out_pixels(musica_ctx* c, uint32_t idx, uint8_t* dst) {
    ABI_TRY
    CHECK_CTX(c); CHECK_IMG(c, idx);
    if (!dst) return fail("musica_get_out_pixels: dst is NULL");
    const uint8_t* px = out_pixels_pinned(c, idx);
    if (!px) return 0;
    const size_t nw = (size_t)c->N - 2 * MUSICA_OUT_MARGIN;
    memcpy(dst, px, nw * nw);
    return 1;
    ABI_CATCH("musica_get_out_pixels")
}

int musica_save_out_image(musica_ctx* c, uint32_t idx, const char* path) {
    ABI_TRY
    CHECK_CTX(c); CHECK_IMG(c, idx);
    if (!path) return fail("musica_save_out_image: path is NULL");
    const uint32_t N = (uint32_t)c->N, margin = MUSICA_OUT_MARGIN;
    if (N <= 2 * margin) return fail("saveOutImage: image too small for the %u-pixel margin", margin);
    const uint32_t nw = N - 2 * margin;
    // The file image is built where it is written from: header by the host, pixel array (24 bpp, bottom-up, padded rows: stbi_write_bmp's
    // layout) by the device straight into page-locked memory, then ONE write — instead of 1 byte per pixel read back, expanded to 3 bytes row
    // by row on the host and written through stdio (26 - 29 ms -> the sum below at 3072^2). MUSICA_SAVE_ON_DEVICE=0: the former path.
    Tick tick("save");
    if (env_int("MUSICA_SAVE_ON_DEVICE", 1) != 0) {
        uint8_t hdr[54];
        const size_t row_bytes = musica_bmp24_header(nw, nw, hdr), file_bytes = 54 + row_bytes * nw;
        if (!c->h_bmp && hipHostMalloc((void**)&c->h_bmp, 2 + file_bytes, hipHostMallocMapped) != hipSuccess) { c->h_bmp = nullptr; (void)hipGetLastError(); }
        void* dev = nullptr;
        if (c->h_bmp && hipHostGetDevicePointer(&dev, c->h_bmp, 0) == hipSuccess && dev) {
            tick.lap("page-locked file image");
            memcpy(c->h_bmp + 2, hdr, 54);
            launch_out_bmp24(c->stream, image_slice(c, c->d_graded, idx), c->lv[0], (int)margin, reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(dev) + 56));
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return fail("saveOutImage: pixel kernel failed: %s", hipGetErrorString(e));
            tick.lap("crop + quantise + 24-bpp rows over the link");
            if (!musica_write_file(path, c->h_bmp + 2, file_bytes)) return fail("failed to write out file");  // :2636-2642
            tick.lap("bmp file");
            return 1;
        }
        (void)hipGetLastError();
    }
    const uint8_t* px = out_pixels_pinned(c, idx);
    if (!px) return 0;
    if (!musica_write_bmp_gray(path, nw, nw, px)) return fail("failed to write out file");  // :2636-2642
    tick.lap("bmp file");
    return 1;
    ABI_CATCH("musica_save_out_image")
}

int musica_get_noise_hist(musica_ctx* c, uint32_t idx, uint32_t level, uint32_t* dst) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    if ((int)level >= c->L) return fail("musica_get_noise_hist: level %u >= %d", level, c->L);
    if (level > MUSICA_CNR_LEVEL) { memset(dst, 0, MUSICA_NOISE_BINS * sizeof(uint32_t)); return 1; }  // cleared, never filled
    return download_small(c, image_slice(c, c->d_noise_hist, idx) + (size_t)level * MUSICA_NOISE_BINS, dst, MUSICA_NOISE_BINS);
}
int musica_get_grad_hist(musica_ctx* c, uint32_t idx, uint32_t* dst) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    return download_small(c, image_slice(c, c->d_grad_hist, idx), dst, MUSICA_GRAD_BINS);
}
int musica_get_noise_hist_max(musica_ctx* c, uint32_t idx, uint32_t level, musica_hist_max_point* dst) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    if ((int)level >= c->L) return fail("musica_get_noise_hist_max: level %u >= %d", level, c->L);
    return download_small(c, image_slice(c, c->d_noise_max, idx) + level, dst, 1);
}
int musica_get_grad_hist_max(musica_ctx* c, uint32_t idx, musica_hist_max_point* dst) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    return download_small(c, image_slice(c, c->d_grad_max, idx), dst, 1);
}
int musica_get_contrast_curve(musica_ctx* c, uint32_t idx, uint32_t level, musica_contrast_curve* dst) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    if ((int)level >= c->L) return fail("musica_get_contrast_curve: level %u >= %d", level, c->L);
    DevCurve dc;
    if (!download_small(c, image_slice(c, c->d_curves, idx) + level, &dc, 1)) return 0;
    memset(dst, 0, sizeof(*dst));
    for (uint32_t i = 0; i < dc.count && i < MUSICA_MAX_POINTS; i++) { dst->points[i].x = dc.x[i]; dst->points[i].y = dc.y[i]; }
    dst->pointsCount = dc.count;
    return 1;
}
int musica_get_grad_curve(musica_ctx* c, uint32_t idx, musica_grad_curve* dst) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    DevCurve dc;
    if (!download_small(c, image_slice(c, c->d_gcurve, idx), &dc, 1)) return 0;
    memset(dst, 0, sizeof(*dst));
    for (uint32_t i = 0; i < dc.count && i < MUSICA_MAX_POINTS; i++) { dst->points[i].x = dc.x[i]; dst->points[i].y = dc.y[i]; }
    dst->pointsCount = dc.count;
    dst->t0 = dc.t0; dst->ta = dc.ta; dst->t1 = dc.t1;
    return 1;
}
// The RENDER_HISTS plots (kernels_gradation.hip k_render_*): rendered into d_plot on the ctx stream, copied out.
static int plot_out(musica_ctx* c, uint8_t* rgba) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(rgba, c->d_plot, (size_t)MUSICA_HIST_RENDER_WIDTH * MUSICA_HIST_RENDER_HEIGHT * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail("plot read-back failed: %s", hipGetErrorString(e));
    return 1;
}
int musica_render_noise_hist(musica_ctx* c, uint32_t idx, uint8_t* rgba) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    if (!rgba) return fail("musica_render_noise_hist: rgba is NULL");
    launch_render_noise_hist(c->stream, image_slice(c, c->d_noise_hist, idx) + MUSICA_CNR_LEVEL * MUSICA_NOISE_BINS,
                             image_slice(c, c->d_noise_max, idx) + MUSICA_CNR_LEVEL, c->d_plot);   // src/vk_processing.cpp:1260-1266
    return plot_out(c, rgba);
}
int musica_render_grad_hist(musica_ctx* c, uint32_t idx, uint8_t* rgba) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    if (!rgba) return fail("musica_render_grad_hist: rgba is NULL");
    launch_render_grad_hist(c->stream, image_slice(c, c->d_grad_hist, idx), image_slice(c, c->d_grad_max, idx), image_slice(c, c->d_gcurve, idx), c->d_plot);   // :1668-1675
    return plot_out(c, rgba);
}
int musica_get_contrast_params(musica_ctx* c, uint32_t level, musica_contrast_params* dst) {
    if (!c || (int)level >= c->L) return fail("musica_get_contrast_params: bad ctx/level");
    *dst = c->h_cparams[level];
    return 1;
}
int musica_get_nr_params(musica_ctx* c, uint32_t level, musica_nr_params* dst) {
    if (!c || level >= 3) return fail("musica_get_nr_params: bad ctx/level");
    *dst = c->h_nr[level];
    return 1;
}
int musica_get_minmax(musica_ctx* c, uint32_t idx, float* min_sqrt, float* max_sqrt) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    uint32_t mm[2];
    const uint32_t* minmax = image_slice(c, c->d_minmax, idx);
    if (!download_small(c, minmax, &mm[0], 1)) return 0;
    if (!download_small(c, minmax + kMaxWord, &mm[1], 1)) return 0;
    // same scalars the normalize kernel derives (kernels_analysis.hip chain_scalars)
    const float mx = sqrtf((float)mm[1]), mn = sqrtf((float)mm[0]);
    *max_sqrt = (float)(uint32_t)mx;
    *min_sqrt = c->min_chain_exact ? (float)(uint32_t)mn : 0.0f;
    return 1;
}
int musica_stats_device_strided(musica_ctx* c, void* d_dst, uint32_t image_id_base, uint32_t image_id_stride) {
    CHECK_CTX(c);
    if (!d_dst) return fail("musica_stats_device: d_dst is NULL");
    launch_stats(c->stream, c->d_cnr, c->lv[MUSICA_CNR_LEVEL], c->d_minmax, c->min_chain_exact, c->d_noise_max, c->L, c->d_grad_max,
                 c->d_gcurve, (musica_stats*)d_dst, image_id_base, image_id_stride, c->B, c->d_stats_partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("kernel launch failed: %s", hipGetErrorString(e));
    return 1;
}
int musica_stats_device(musica_ctx* c, void* d_dst, uint32_t image_id_base) { return musica_stats_device_strided(c, d_dst, image_id_base, 1u); }

// ---- device-resident output and stream ordering (musica_export_out, musica_stream_wait / _signal) ----------------------------------------
// Everything about the destination is checked on the host before anything is enqueued: a kernel store to pageable host memory faults the
// GPU, and a store past the end of the caller's allocation lands in whatever the runtime placed behind it.
int musica_export_out(musica_ctx* c, uint32_t first, uint32_t count, uint32_t format, void* d_dst, size_t row_pitch, size_t image_pitch) {
    CHECK_CTX(c);
    if (!d_dst) return fail("musica_export_out: d_dst is NULL");
    {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, d_dst) != hipSuccess) {
            (void)hipGetLastError();
            return fail("musica_export_out: d_dst is not device memory (the HIP runtime does not know it: pageable host memory?)");
        }
        if (a.type != hipMemoryTypeDevice) return fail("musica_export_out: d_dst is not device memory (memory type %d)", (int)a.type);
        if (a.device != c->p.device) return fail("musica_export_out: d_dst is memory of device %d, the context runs on device %d", a.device, c->p.device);
    }
    if (format >= MUSICA_OUT_FORMAT_COUNT) return fail("musica_export_out: format %u out of range", format);
    if (count == 0) return fail("musica_export_out: count is 0");
    if ((uint64_t)first + count > (uint64_t)c->B) return fail("musica_export_out: images %u .. %u + %u exceed the batch of %d", first, first, count, c->B);
    const bool u8 = format == MUSICA_OUT_U8;
    if (u8 && c->N <= 2 * MUSICA_OUT_MARGIN) return fail("musica_export_out: image too small for the %d-pixel margin", MUSICA_OUT_MARGIN);
    const size_t rows = u8 ? (size_t)c->N - 2 * MUSICA_OUT_MARGIN : (size_t)c->N;
    const size_t width = u8 ? rows : (size_t)c->N * sizeof(float);
    size_t image_bytes = 0, last = 0;
    if (row_pitch < width) return fail("musica_export_out: row pitch %zu below the %zu bytes of a row", row_pitch, width);
    if (__builtin_mul_overflow(row_pitch, rows, &image_bytes) || image_pitch < image_bytes)
        return fail("musica_export_out: image pitch %zu below the %zu rows of pitch %zu", image_pitch, rows, row_pitch);
    if (!u8 && (((uintptr_t)d_dst | row_pitch | image_pitch) & 3u) != 0)
        return fail("musica_export_out: MUSICA_OUT_GRADED_F32 wants d_dst and both pitches on a multiple of 4 bytes");
    if (!c->stepped) return fail("musica_export_out: no step has run on this context");
    {
        // the last byte written: image count - 1, row rows - 1, byte width - 1
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, d_dst) != hipSuccess) {
            (void)hipGetLastError();
            return fail("musica_export_out: the allocation that holds d_dst is unknown");
        }
        const size_t room = (size_t)((uintptr_t)base + size - (uintptr_t)d_dst);   // bytes from d_dst to the end of its allocation
        if (__builtin_mul_overflow((size_t)(count - 1), image_pitch, &last) || __builtin_add_overflow(last, image_bytes - row_pitch + width, &last) ||
            last > room)
            return fail("musica_export_out: %u images of pitch %zu (rows of pitch %zu) reach beyond the allocation that holds d_dst (%zu bytes from d_dst)",
                        count, image_pitch, row_pitch, room);
    }
    const float* src = image_slice(c, c->d_graded, first);
    if (u8) {
        launch_export_u8(c->stream, src, c->lv[0], (int)count, (uint8_t*)d_dst, row_pitch, image_pitch);
    } else {
        // a pitched device-to-device copy; one over every image when the destination's images follow each other at its row pitch (the
        // graded planes do: a plane is exactly N rows of the level-0 pitch)
        const size_t spitch = (size_t)c->lv[0].pitch * sizeof(float);
        if (image_pitch == image_bytes && per_image(c, c->d_graded) == c->lv[0].plane) {
            HIP_OK(hipMemcpy2DAsync(d_dst, row_pitch, src, spitch, width, rows * count, hipMemcpyDeviceToDevice, c->stream));
        } else {
            for (uint32_t k = 0; k < count; k++)
                HIP_OK(hipMemcpy2DAsync((uint8_t*)d_dst + (size_t)k * image_pitch, row_pitch, image_slice(c, c->d_graded, first + k), spitch, width, rows,
                                        hipMemcpyDeviceToDevice, c->stream));
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("musica_export_out: launch failed: %s", hipGetErrorString(e));
    return 1;
}

// A caller's stream: of the context's device and not capturing (a graph captured from the caller's side must not take in the context's
// stream, and the events below are recorded eagerly).
static int check_caller_stream(musica_ctx* c, hipStream_t s, const char* fn) {
    hipDevice_t dev = -1;
    if (hipStreamGetDevice(s, &dev) != hipSuccess) { (void)hipGetLastError(); return fail("%s: not a stream of this process", fn); }
    if (dev != c->p.device) return fail("%s: the stream belongs to device %d, the context runs on device %d", fn, (int)dev, c->p.device);
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return fail("%s: the stream's capture status is unknown", fn); }
    if (st != hipStreamCaptureStatusNone) return fail("%s: the stream is capturing a graph (capturing these calls is not supported)", fn);
    return 1;
}
static int caller_events(musica_ctx* c) {
    if (c->ev_signal) return 1;   // keyed on the LAST resource of the block: a call that failed half-way is retried, never half-initialised
    if (!c->ev_caller) HIP_OK(hipEventCreateWithFlags(&c->ev_caller, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&c->ev_signal, hipEventDisableTiming));
    return 1;
}
int musica_stream_wait(musica_ctx* c, void* stream) {
    CHECK_CTX(c);
    const hipStream_t s = (hipStream_t)stream;
    if (!check_caller_stream(c, s, "musica_stream_wait") || !caller_events(c)) return 0;
    HIP_OK(hipEventRecord(c->ev_caller, s));
    HIP_OK(hipStreamWaitEvent(c->stream, c->ev_caller, 0));
    return 1;
}
int musica_stream_signal(musica_ctx* c, void* stream) {
    CHECK_CTX(c);
    const hipStream_t s = (hipStream_t)stream;
    if (!check_caller_stream(c, s, "musica_stream_signal") || !caller_events(c)) return 0;
    // a two-stream step's side stream has rejoined c->stream (ev_join) before its last launches, and a replayed graph completes as a whole
    // before anything behind it on c->stream: this event covers all of it
    HIP_OK(hipEventRecord(c->ev_signal, c->stream));
    HIP_OK(hipStreamWaitEvent(s, c->ev_signal, 0));
    return 1;
}
int musica_get_stats(musica_ctx* c, uint32_t idx, musica_stats* dst) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    if (!musica_stats_device(c, c->d_stats, 0)) return 0;
    return download_small(c, image_slice(c, c->d_stats, idx), dst, 1);
}
int musica_get_clahe_hist(musica_ctx* c, uint32_t idx, uint32_t* dst) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    if (!c->d_clahe_hist) return fail("musica_get_clahe_hist: ctx was created without MUSICA_FLAG_CLAHE");
    return download_small(c, image_slice(c, c->d_clahe_hist, idx), dst, per_image(c, c->d_clahe_hist));
}
int musica_get_clahe_curves(musica_ctx* c, uint32_t idx, musica_point* dst) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    if (!c->d_clahe_pts) return fail("musica_get_clahe_curves: ctx was created without MUSICA_FLAG_CLAHE");
    return download_small(c, image_slice(c, c->d_clahe_pts, idx), dst, per_image(c, c->d_clahe_pts));
}

// VulkanState::downloadAndSaveImage (src/vk_state.cpp:809-855): (uint8_t)(255 * (v - min) / (max - min)), full image.
static int dump_image(musica_ctx* c, uint32_t idx, musica_image_kind kind, uint32_t level, const std::string& path, float maxValue, float minValue) {
    const uint32_t side = musica_image_side(c, kind, level);
    std::vector<float> img((size_t)side * side);
    if (!musica_get_image(c, idx, kind, level, img.data())) return 0;
    std::vector<uint8_t> out((size_t)side * side);
    for (size_t i = 0; i < out.size(); i++) {
        const float q = 255.0f * (img[i] - minValue) / (maxValue - minValue);
        // the reference's C cast is undefined outside [0, 256); wrap like the common x86 lowering (cvttss2si + truncate)
        out[i] = (q == q && q > -2147483648.0f && q < 2147483648.0f) ? (uint8_t)(int32_t)q : 0;
    }
    if (!musica_write_bmp_gray(path.c_str(), side, side, out.data())) return fail("failed to write %s", path.c_str());
    return 1;
}

int musica_debug_process(musica_ctx* c, uint32_t idx, const char* dir) {
    CHECK_CTX(c); CHECK_IMG(c, idx);
    ABI_TRY
    const std::string d = std::string(dir && *dir ? dir : ".") + "/";
    if (!dump_image(c, idx, MUSICA_IMG_NORMALIZED, 0, d + "norm.bmp", 1.0f, 0.0f)) return 0;               // :2664-2671
    for (int i = 0; i < c->L; i++) {                                                                       // :2673-2690
        if (!dump_image(c, idx, MUSICA_IMG_BANDPASS, i, d + "red_bandpass_" + std::to_string(i) + ".bmp", 1.0f, -1.0f)) return 0;
        if (!dump_image(c, idx, MUSICA_IMG_LOWPASS, i, d + "red_lowpass_" + std::to_string(i) + ".bmp", 1.0f, 0.0f)) return 0;
    }
    if (!dump_image(c, idx, MUSICA_IMG_SDEV, MUSICA_CNR_LEVEL, d + "sdev.bmp", 1.0f, -1.0f)) return 0;      // :2692-2699
    if (!dump_image(c, idx, MUSICA_IMG_CNR, MUSICA_CNR_LEVEL, d + "cnr.bmp", 1.0f, 0.0f)) return 0;         // :2701-2708
    for (int i = 0; i < c->L; i++) {                                                                       // :2710-2727 (slot i <-> level L-1-i)
        const int lvl = c->L - 1 - i;
        // expandBandpassImageStates[i]: the contrast-curve output, before noise reduction (src/vk_processing.cpp:1100)
        if (!dump_image(c, idx, MUSICA_IMG_CONTRAST_BAND, lvl, d + "exp_bandpass_" + std::to_string(i) + ".bmp", 1.0f, -1.0f)) return 0;
        // expandLowpassImageStates[i] = smooth_upsampled(upsample(previous reconstruction))
        const LevelDesc& lf = c->lv[lvl];
        const float* prev = lvl == c->L - 1 ? c->d_down[c->L - 1] : c->d_recon[lvl + 1];
        launch_lowpass(c->stream, prev, c->d_scratch, lf, c->lv[lvl + 1], c->B, c->ref_order);
        std::vector<float> img((size_t)lf.S * lf.S);
        if (!download_plane(c, c->d_scratch + (size_t)idx * lf.plane, lf, img.data())) return 0;
        std::vector<uint8_t> out(img.size());
        for (size_t k = 0; k < out.size(); k++) {
            const float q = 255.0f * img[k];
            out[k] = (q == q && q > -2147483648.0f && q < 2147483648.0f) ? (uint8_t)(int32_t)q : 0;
        }
        if (!musica_write_bmp_gray((d + "exp_lowpass_" + std::to_string(i) + ".bmp").c_str(), lf.S, lf.S, out.data())) return fail("failed to write exp_lowpass");
    }
    if (!dump_image(c, idx, MUSICA_IMG_RELEVANT, 0, d + "relevant.bmp", 1.0f, 0.0f)) return 0;              // :2729-2736
    if (!dump_image(c, idx, MUSICA_IMG_GRADED, 0, d + "graded.bmp", 1.0f, 0.0f)) return 0;                  // :2749-2756
    {   // the two RGBA plots, :2758-2806
        std::vector<uint8_t> plot((size_t)MUSICA_HIST_RENDER_WIDTH * MUSICA_HIST_RENDER_HEIGHT * 4);
        if (!musica_render_noise_hist(c, idx, plot.data())) return 0;
        if (!musica_write_bmp_rgba((d + "noise_hist.bmp").c_str(), MUSICA_HIST_RENDER_WIDTH, MUSICA_HIST_RENDER_HEIGHT, plot.data())) return fail("failed to write noise_hist.bmp");
        if (!musica_render_grad_hist(c, idx, plot.data())) return 0;
        if (!musica_write_bmp_rgba((d + "grad_hist.bmp").c_str(), MUSICA_HIST_RENDER_WIDTH, MUSICA_HIST_RENDER_HEIGHT, plot.data())) return fail("failed to write grad_hist.bmp");
    }
    // and the numbers behind them as CSV (an addition)
    {
        std::vector<uint32_t> h(MUSICA_NOISE_BINS);
        FILE* f = fopen((d + "noise_hist.csv").c_str(), "w");
        if (!f) return fail("failed to write noise_hist.csv");
        fprintf(f, "bin,level0,level1,level2,level3\n");
        std::vector<uint32_t> all(4 * MUSICA_NOISE_BINS);
        for (uint32_t l = 0; l < 4; l++)
            if (!musica_get_noise_hist(c, idx, l, all.data() + l * MUSICA_NOISE_BINS)) { fclose(f); return 0; }
        for (int b = 0; b < MUSICA_NOISE_BINS; b++)
            fprintf(f, "%d,%u,%u,%u,%u\n", b, all[b], all[MUSICA_NOISE_BINS + b], all[2 * MUSICA_NOISE_BINS + b], all[3 * MUSICA_NOISE_BINS + b]);
        fclose(f);
    }
    {
        std::vector<uint32_t> h(MUSICA_GRAD_BINS);
        if (!musica_get_grad_hist(c, idx, h.data())) return 0;
        musica_grad_curve gc;
        if (!musica_get_grad_curve(c, idx, &gc)) return 0;
        FILE* f = fopen((d + "grad_hist.csv").c_str(), "w");
        if (!f) return fail("failed to write grad_hist.csv");
        fprintf(f, "bin,weight\n");
        for (int b = 0; b < MUSICA_GRAD_BINS; b++) fprintf(f, "%d,%u\n", b, h[b]);
        fclose(f);
        f = fopen((d + "grad_curve.csv").c_str(), "w");
        if (!f) return fail("failed to write grad_curve.csv");
        fprintf(f, "# t0=%.9g ta=%.9g t1=%.9g\nx,y\n", gc.t0, gc.ta, gc.t1);
        for (uint32_t i = 0; i < gc.pointsCount; i++) fprintf(f, "%.9g,%.9g\n", gc.points[i].x, gc.points[i].y);
        fclose(f);
    }
    return 1;
    ABI_CATCH("musica_debug_process")
}

// ---- profiling ------------------------------------------------------------------------
int musica_profile_enable(musica_ctx* c, int enabled) {
    CHECK_CTX(c);
    HIP_OK(hipStreamSynchronize(c->stream));
    collect_spans(c);
    c->profiling = enabled < 0 ? 0xFFFFFFFFu : (uint32_t)enabled;  // < 0: every kernel family; else bit i = musica_kernel_id i
    return 1;
}
int musica_profile_reset(musica_ctx* c) {
    CHECK_CTX(c);
    HIP_OK(hipStreamSynchronize(c->stream));
    c->spans_used = 0;
    memset(c->prof_total_us, 0, sizeof(c->prof_total_us));
    memset(c->prof_count, 0, sizeof(c->prof_count));
    return 1;
}
int musica_profile_get(musica_ctx* c, musica_kernel_id id, double* mean_us, uint64_t* launches) {
    CHECK_CTX(c);
    if ((int)id < 0 || id >= MUSICA_KERNEL_COUNT) return fail("musica_profile_get: bad kernel id %d", (int)id);
    if (mean_us) *mean_us = c->prof_count[id] ? c->prof_total_us[id] / (double)c->prof_count[id] : 0.0;
    if (launches) *launches = c->prof_count[id];
    return 1;
}

// ---- stand-alone metric kernel ----------------------------------------------------------
static int reduce_descs(uint32_t side, uint32_t in_pitch, uint32_t out_pitch, LevelDesc* li, LevelDesc* lo) {
    if (side < 1) return fail("musica_k_reduce: side must be >= 1");
    const uint32_t so = (side + 1) / 2;
    if (in_pitch < side || (in_pitch & 3) || out_pitch < so || (out_pitch & 3)) return fail("musica_k_reduce: pitches must be multiples of 4 floats and cover the rows");
    li->S = (int)side; li->pitch = (int)in_pitch; li->plane = (size_t)in_pitch * side;
    lo->S = (int)so; lo->pitch = (int)out_pitch; lo->plane = (size_t)out_pitch * so;
    return 1;
}

int musica_k_reduce(musica_ctx* c, const float* d_in, uint32_t side, uint32_t in_pitch, float* d_out, uint32_t out_pitch, uint32_t batch) {
    CHECK_CTX(c);
    LevelDesc li, lo;
    if (!reduce_descs(side, in_pitch, out_pitch, &li, &lo)) return 0;
    launch_reduce(c->stream, d_in, li, d_out, lo, (int)batch, c->generic, 2, c->xcd_swizzle, c->xcd_regions);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("kernel launch failed: %s", hipGetErrorString(e));
    return 1;
}

int musica_selftest_exact_math(musica_ctx* c, uint64_t mismatches[4]) {
    CHECK_CTX(c);
    if (!mismatches) return fail("musica_selftest_exact_math: mismatches is NULL");
    unsigned long long* d = nullptr;
    HIP_OK(hipMalloc(&d, 4 * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, 4 * sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) {
        launch_selftest_exact_math(c->stream, d);
        e = hipStreamSynchronize(c->stream);
    }
    unsigned long long h[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) return fail("musica_selftest_exact_math: %s", hipGetErrorString(e));
    for (int i = 0; i < 4; i++) mismatches[i] = h[i];
    return 1;
}

int musica_k_reduce_timed(musica_ctx* c, const float* d_in, uint32_t side, uint32_t in_pitch, float* d_out, uint32_t out_pitch, uint32_t batch,
                          uint32_t iters, double* mean_us) {
    CHECK_CTX(c);
    LevelDesc li, lo;
    if (!reduce_descs(side, in_pitch, out_pitch, &li, &lo)) return 0;
    if (iters < 1) iters = 1;
    hipEvent_t a, b;
    HIP_OK(hipEventCreate(&a));
    HIP_OK(hipEventCreate(&b));
    HIP_OK(hipEventRecord(a, c->stream));
    for (uint32_t i = 0; i < iters; i++) launch_reduce(c->stream, d_in, li, d_out, lo, (int)batch, c->generic, 2, c->xcd_swizzle, c->xcd_regions);
    HIP_OK(hipEventRecord(b, c->stream));
    HIP_OK(hipEventSynchronize(b));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, a, b));
    hipEventDestroy(a);
    hipEventDestroy(b);
    if (mean_us) *mean_us = (double)ms * 1000.0 / (double)iters;
    return 1;
}

int musica_k_reduce_timed_rot(musica_ctx* c, const float* d_in, uint32_t side, uint32_t in_pitch, float* d_out, uint32_t out_pitch, uint32_t nbuf,
                              uint32_t iters, double* mean_us) {
    CHECK_CTX(c);
    LevelDesc li, lo;
    if (!reduce_descs(side, in_pitch, out_pitch, &li, &lo)) return 0;
    if (iters < 1) iters = 1;
    if (nbuf < 1) nbuf = 1;
    hipEvent_t a, b;
    HIP_OK(hipEventCreate(&a));
    HIP_OK(hipEventCreate(&b));
    HIP_OK(hipEventRecord(a, c->stream));
    for (uint32_t i = 0; i < iters; i++)
        launch_reduce(c->stream, d_in + (size_t)(i % nbuf) * li.plane, li, d_out + (size_t)(i % nbuf) * lo.plane, lo, 1, c->generic, side <= 4096 ? 4 : 5, c->xcd_swizzle, c->xcd_regions);
    HIP_OK(hipEventRecord(b, c->stream));
    HIP_OK(hipEventSynchronize(b));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, a, b));
    hipEventDestroy(a);
    hipEventDestroy(b);
    if (mean_us) *mean_us = (double)ms * 1000.0 / (double)iters;
    return 1;
}

int musica_k_copy41_timed_rot(musica_ctx* c, const float* d_in, uint32_t side, float* d_out, uint32_t nbuf, uint32_t iters, double* mean_us) {
    CHECK_CTX(c);
    if (side < 8 || (side & 7)) return fail("musica_k_copy41_timed_rot: side must be a multiple of 8");
    if (iters < 1) iters = 1;
    if (nbuf < 1) nbuf = 1;
    const size_t in_plane = (size_t)side * side, out_plane = in_plane / 4;
    hipEvent_t a, b;
    HIP_OK(hipEventCreate(&a));
    HIP_OK(hipEventCreate(&b));
    HIP_OK(hipEventRecord(a, c->stream));
    for (uint32_t i = 0; i < iters; i++) launch_copy41(c->stream, d_in + (size_t)(i % nbuf) * in_plane, d_out + (size_t)(i % nbuf) * out_plane, (int)side);
    HIP_OK(hipEventRecord(b, c->stream));
    HIP_OK(hipEventSynchronize(b));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, a, b));
    hipEventDestroy(a);
    hipEventDestroy(b);
    if (mean_us) *mean_us = (double)ms * 1000.0 / (double)iters;
    return 1;
}

void* musica_device_alloc(musica_ctx* c, size_t bytes) {
    if (!c || hipSetDevice(c->p.device) != hipSuccess) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { fail("musica_device_alloc(%zu) failed", bytes); return nullptr; }
    return p;
}
void musica_device_free(musica_ctx* c, void* p) {
    if (!c || !p) return;
    hipSetDevice(c->p.device);
    hipStreamSynchronize(c->stream);
    hipFree(p);
}
int musica_memcpy_h2d(musica_ctx* c, void* d_dst, const void* src, size_t bytes) {
    CHECK_CTX(c);
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return 1;
}
int musica_memcpy_d2h(musica_ctx* c, void* dst, const void* d_src, size_t bytes) {
    CHECK_CTX(c);
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return 1;
}

}  // extern "C"
